"""float64 numpy restatements of the doublet-aware clustering: the doublet likelihood LLD[b][r][p] of the pairs
(k, l), k < l, of every restart's clusters, and the E-step over K singlet and P doublet components.  No GPU and no engine needed."""
import numpy as np


def pairs(K):
    """[P][2]: (k, l), k < l, lexicographic."""
    return np.array([(k, l) for k in range(K) for l in range(k + 1, K)], dtype=np.int64).reshape(-1, 2)


def pair_pg(nrd, start, reads, mat, err):
    """float64 [P][5]: the reference's doublet factors at alpha = 0.5 (cmd_cram_demuxlet.cpp:594-663, weight s / 4) for every stored
    pair, reads in stored order, vectorised over pairs."""
    n = len(nrd)
    w = np.arange(5) / 4.0
    G = np.ones((n, 5))
    for r in range(int(nrd.max()) if n else 0):
        idx = np.flatnonzero(nrd > r)
        b = reads[start[idx] + r].astype(np.int64)
        bq, alt = b & 127, (b >> 7) != 0
        pR = np.where(alt, err[bq] / 3.0, mat[bq])
        pA = np.where(alt, mat[bq], err[bq] / 3.0)
        G[idx] *= pR[:, None] * (1.0 - w)[None, :] + pA[:, None] * w[None, :]
        G[idx] /= G[idx].max(axis=1, keepdims=True)
    G = G + 1e-6
    return G / G.max(axis=1, keepdims=True)


def lld(sp, g, R, K, mat, err):
    """LLD[B][R][P] of a synth pileup `sp` (cell_pair_off, pair_snp or None = dense, pair_nrd, reads) and a genotype matrix
    g[S][R * K][3]: per pair, log(sum over x, y of g_k[x] g_l[y] pG[x + y]), summed over the barcode's pairs.  Also lsc[B]: the sum
    over the barcode's pairs of log(pG[0] + pG[2] + pG[4]).  Returns (LLD, lsc)."""
    B = sp.n_cells
    po = np.asarray(sp.cell_pair_off, dtype=np.int64)
    cell = np.repeat(np.arange(B), np.diff(po))
    snp = np.asarray(sp.pair_snp, dtype=np.int64) if sp.pair_snp is not None else np.arange(len(cell)) - po[cell]
    nrd = np.asarray(sp.pair_nrd, dtype=np.int64)
    start = np.cumsum(nrd) - nrd
    pG = pair_pg(nrd, start, np.asarray(sp.reads), mat, err)
    pr = pairs(K)
    g = np.asarray(g, dtype=np.float64).reshape(g.shape[0], R, K, 3)
    out = np.zeros((B, R, len(pr)))
    H = np.zeros((5, 3, 3))
    for x in range(3):
        for y in range(3):
            H[x + y, x, y] = 1.0
    M = np.einsum("ps,sxy->pxy", pG, H)                      # [pairs][3][3]: pG[x + y]
    for r in range(R):
        gk = g[snp][:, r, pr[:, 0], :]                       # [pairs][P][3]
        gl = g[snp][:, r, pr[:, 1], :]
        L = np.einsum("npx,nxy,npy->np", gk, M, gl)
        np.add.at(out[:, r, :], cell, np.log(L))
    lsc = np.zeros(B)
    np.add.at(lsc, cell, np.log(pG[:, 0] + pG[:, 2] + pG[:, 4]))
    return out, lsc


def log_priors(log_pi, log_delta):
    """(lps[R][K], lpd[R][P]): singlet log(1 - delta) + log pi_k, doublet log delta + log(2 pi_k pi_l / (1 - sum pi^2))."""
    log_pi = np.asarray(log_pi, dtype=np.float64)
    R, K = log_pi.shape
    ld = np.asarray(log_delta, dtype=np.float64).reshape(R)
    pr = pairs(K)
    lps = log_pi + np.log1p(-np.exp(ld))[:, None]
    s2 = np.exp(2.0 * log_pi).sum(axis=1)
    with np.errstate(divide="ignore"):
        lpd = ld[:, None] + np.log(2.0) + log_pi[:, pr[:, 0]] + log_pi[:, pr[:, 1]] - np.log1p(-s2)[:, None]
    lpd[np.isneginf(ld)] = -np.inf
    return lps, lpd


def estep(llks, lld_, log_pi, log_delta, T=1.0, mask=None):
    """The doublet E-step.  llks[B][R * K], lld_[B][R][P] the doublet likelihoods on the singlets' scale (the engine's LLD - lsc).  Returns (w[B][R * K], dm[B][R], ll[R], col_sum[R * K], dbl_mass[R]):
    w the singlet posteriors, dm the doublet mass per barcode; barcodes outside the mask get zeros and no part in the sums."""
    log_pi = np.asarray(log_pi, dtype=np.float64)
    R, K = log_pi.shape
    B = llks.shape[0]
    lps, lpd = log_priors(log_pi, log_delta)
    xs = llks.reshape(B, R, K) + lps[None]
    xd = lld_ + lpd[None]
    x = np.concatenate([xs, xd], axis=2)                     # [B][R][K + P]
    a = x / T
    m = a.max(axis=2, keepdims=True)
    e = np.exp(a - m)
    z = e.sum(axis=2, keepdims=True)
    w = e[:, :, :K] / z
    dm = e[:, :, K:].sum(axis=2) / z[:, :, 0]
    m1 = x.max(axis=2, keepdims=True)
    lse = m1[:, :, 0] + np.log(np.exp(x - m1).sum(axis=2))
    keep = np.ones(B, bool) if mask is None else np.asarray(mask, dtype=bool)
    w[~keep] = 0.0
    dm[~keep] = 0.0
    w = w.reshape(B, R * K)
    return w, dm, lse[keep].sum(axis=0), w.sum(axis=0), dm.sum(axis=0)


def estep_plain(llks, log_pi, T=1.0, mask=None):
    """The singlet-only E-step of section 13 (dmx_engine_cluster_estep): (w[B][R * K], ll[R], col_sum[R * K])."""
    log_pi = np.asarray(log_pi, dtype=np.float64)
    R, K = log_pi.shape
    B = llks.shape[0]
    x = llks.reshape(B, R, K) + log_pi[None]
    a = x / T
    w = np.exp(a - a.max(axis=2, keepdims=True))
    w /= w.sum(axis=2, keepdims=True)
    lse = x.max(axis=2) + np.log(np.exp(x - x.max(axis=2, keepdims=True)).sum(axis=2))
    keep = np.ones(B, bool) if mask is None else np.asarray(mask, dtype=bool)
    w[~keep] = 0.0
    w = w.reshape(B, R * K)
    return w, lse[keep].sum(axis=0), w.sum(axis=0)
