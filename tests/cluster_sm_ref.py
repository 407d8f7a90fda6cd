"""float64 numpy restatements of the split-merge moves' device parts: the merge scores of every pair of a
restart's clusters from an M-step's LL / W, and the grouped E-step.  No GPU and no engine needed."""
import numpy as np


def pairs(K):
    """[P][2]: (k, l), k < l, lexicographic."""
    return np.array([(k, l) for k in range(K) for l in range(k + 1, K)], dtype=np.int64).reshape(-1, 2)


def lse3(x):
    m = x.max(axis=-1, keepdims=True)
    return m[..., 0] + np.log(np.exp(x - m).sum(axis=-1))


def merge_score(LL, W, q, floor, R, K):
    """(bf[R][P], n_shared[R][P]) for LL[S][R*K][3], W[S][R*K], the prior q[S][3] (float32) and floor:
    bf = sum over the SNPs where both W > 0 of lse_g(log pi + LL_k + LL_l) - A_k - A_l, A_c = lse_g(log pi + LL_c)."""
    a = q.astype(np.float64) + floor
    lp = np.log(a / a.sum(axis=1, keepdims=True))                      # [S][3]
    A = lse3(lp[:, None, :] + LL)                                      # [S][C]
    on = W > 0
    pr = pairs(K)
    bf = np.zeros((R, len(pr)))
    ns = np.zeros((R, len(pr)), dtype=np.int64)
    for r in range(R):
        for p, (k, l) in enumerate(pr):
            ck, cl = r * K + k, r * K + l
            both = on[:, ck] & on[:, cl]
            t = lse3(lp + LL[:, ck] + LL[:, cl]) - A[:, ck] - A[:, cl]
            bf[r, p] = t[both].sum()
            ns[r, p] = int(both.sum())
    return bf, ns


def estep_grouped(llks, R, K, log_pi, group, rpg, T=1.0, mask=None):
    """(w[B][R*K], ll[R], col_sum[R*K]): the plain E-step, restart r restricted to the barcodes with group[b] == r // rpg (and in the mask)."""
    B = llks.shape[0]
    x = llks.reshape(B, R, K) + np.asarray(log_pi).reshape(1, R, K)
    a = x / T
    w = np.exp(a - a.max(axis=2, keepdims=True))
    w /= w.sum(axis=2, keepdims=True)
    lse = x.max(axis=2) + np.log(np.exp(x - x.max(axis=2, keepdims=True)).sum(axis=2))
    keep = np.asarray(group)[:, None] == (np.arange(R) // rpg)[None, :]
    if mask is not None:
        keep &= np.asarray(mask, dtype=bool)[:, None]
    w[~keep] = 0.0
    lse[~keep] = 0.0
    w = w.reshape(B, R * K)
    return w, lse.sum(axis=0), w.sum(axis=0)
