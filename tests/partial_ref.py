"""float64 numpy restatement of the partly genotyped pool's E-step and windowed M-step (include/dmx.h
dmx_engine_cluster_estep_known / dmx_engine_cluster_mstep_window)."""
import numpy as np


def llk_columns(R: int, Vk: int, M: int) -> np.ndarray:
    """[R][Vk + M]: the engine column of component k of restart r (k < Vk: k; else Vk + r M + k - Vk)."""
    col = np.empty((R, Vk + M), dtype=np.int64)
    col[:, :Vk] = np.arange(Vk)
    col[:, Vk:] = Vk + np.arange(R)[:, None] * M + np.arange(M)[None, :]
    return col


def estep_known(llks: np.ndarray, R: int, Vk: int, M: int, log_pi: np.ndarray, T: float = 1.0, mask=None):
    """(w[B][R][Vk + M], free w[B][R * M], ll[R], col_sum[R][Vk + M]) from K1's llks[B][Vk + R M]."""
    B = llks.shape[0]
    x = llks[:, llk_columns(R, Vk, M)] + np.asarray(log_pi, dtype=np.float64).reshape(R, Vk + M)[None]
    a = x / T
    w = np.exp(a - a.max(axis=2, keepdims=True))
    w /= w.sum(axis=2, keepdims=True)
    mx = x.max(axis=2, keepdims=True)
    lse = mx[..., 0] + np.log(np.exp(x - mx).sum(axis=2))
    keep = np.ones(B, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    w[~keep] = 0.0
    lse[~keep] = 0.0
    return w, np.ascontiguousarray(w[:, :, Vk:]).reshape(B, R * M), lse.sum(axis=0), w.sum(axis=0)


def mstep_window(off: np.ndarray, cell: np.ndarray, lgl: np.ndarray, w: np.ndarray, q: np.ndarray, floor: float, g_known: np.ndarray):
    """(LL[S][C][3], W[S][C], gp[S][Vk + C][3] f32) for free weights w[B][C] over the stage cache (off, cell, lgl) and prior q[S][3];
    gp's first Vk columns are g_known's rows, a free row without weight is q's."""
    S, C = len(off) - 1, w.shape[1]
    snp = np.repeat(np.arange(S), np.diff(off))
    LL = np.zeros((S, C, 3))
    W = np.zeros((S, C))
    for g in range(3):
        np.add.at(LL[:, :, g], snp, w[cell] * lgl[:, g][:, None])
    np.add.at(W, snp, w[cell])
    qq = q.astype(np.float64)[:, None, :] + floor
    x = qq * np.exp(LL - LL.max(axis=2, keepdims=True))
    gp = (x / x.sum(axis=2, keepdims=True)).astype(np.float32)
    gp = np.where((W > 0)[..., None], gp, np.broadcast_to(q[:, None, :], gp.shape))
    return LL, W, np.concatenate([np.asarray(g_known, dtype=np.float32), gp], axis=1)
