"""float64 numpy restatements of the parts that choose the number of clusters: the evidence of an M-step's
columns, the hard labels with their counts, one-hot matrix and doublet score, the column merge, and the path's score.  No GPU and no
engine needed."""
from math import lgamma

import numpy as np

from cluster_sm_ref import lse3, pairs


def evidence(LL, W, q, floor, R, K):
    """(ev[R][K], n_cov[R][K]) for LL[S][R*K][3], W[S][R*K], the prior q[S][3] (float32) and floor: ev = the sum over the SNPs with
    W > 0 of A = lse_g(log pi + LL), in the device's order (chunks of 256 SNPs serially, then the chunks)."""
    a = q.astype(np.float64) + floor
    lp = np.log(a / a.sum(axis=1, keepdims=True))
    A = np.where(W > 0, lse3(lp[:, None, :] + LL), 0.0)                # [S][C]
    S, C = W.shape
    ev = np.zeros(C)
    for s0 in range(0, S, 256):
        part = np.zeros(C)
        for i in range(s0, min(S, s0 + 256)):
            part = part + A[i]                                         # (a skipped SNP adds +0.0, which changes no bits)
        ev = ev + part
    return ev.reshape(R, K), (W > 0).sum(axis=0).astype(np.int64).reshape(R, K)


def hard(w, active, R, K, mask=None, dbl_mass=None, lld=None):
    """(label[B][R], n_sing[R][K], n_dbl[R], dbl_score[R], hot[B][R*K]) from the weights w[B][R*K], active[R][K] and, for doublet labels,
    the doublet mass dbl_mass[B][R] and LLD[B][R][P]."""
    B = w.shape[0]
    act = np.asarray(active, dtype=bool).reshape(R, K)
    pr = pairs(K)
    label = np.full((B, R), -1, dtype=np.int64)
    dsc = np.zeros((B, R))
    hot = np.zeros((B, R * K))
    for r in range(R):
        ks = np.flatnonzero(act[r])
        ps = np.flatnonzero(act[r][pr[:, 0]] & act[r][pr[:, 1]]) if len(pr) else np.zeros(0, dtype=np.int64)
        for b in range(B):
            if mask is not None and not mask[b]:
                continue
            if dbl_mass is not None and dbl_mass[b, r] >= 0.5:
                p = ps[int(np.argmax(lld[b, r, ps]))]                  # (argmax: the first of the highest)
                label[b, r], dsc[b, r] = -2 - p, lld[b, r, p]
            else:
                k = ks[int(np.argmax(w[b, r * K + ks]))]
                label[b, r] = k
                hot[b, r * K + k] = 1.0
    n_sing = np.array([[int((label[:, r] == k).sum()) for k in range(K)] for r in range(R)], dtype=np.int64).reshape(R, K)
    n_dbl = (label <= -2).sum(axis=0)
    score = np.zeros(R)
    for b0 in range(0, B, 256):
        part = np.zeros(R)
        for b in range(b0, min(B, b0 + 256)):
            part = part + dsc[b]
        score = score + part
    return label, n_sing, n_dbl, score, hot


def merge_columns(w, R, K, frm, into):
    """The weights after w[into] = w[into] + w[from], w[from] = 0 in every restart with from >= 0."""
    out = np.array(w, dtype=np.float64)
    for r in range(R):
        if frm[r] >= 0:
            out[:, r * K + into[r]] = out[:, r * K + into[r]] + out[:, r * K + frm[r]]
            out[:, r * K + frm[r]] = 0.0
    return out


def label_term(n_sing, n_dbl):
    """log P(labels) of one labelling with n_sing[k] singlets in each of the Ka active clusters and n_dbl doublets: which barcodes are
    doublets under a flat Beta on the doublet share, times the singlets' clusters under a flat Dirichlet on the mixing weights."""
    n = [int(x) for x in n_sing]
    ka, ns = len(n), sum(n)
    return (lgamma(ka) + sum(lgamma(x + 1) for x in n) - lgamma(ns + ka)) + (lgamma(n_dbl + 1) + lgamma(ns + 1) - lgamma(ns + n_dbl + 2))


def path_score(ev, n_sing, n_dbl, dbl_score, active):
    act = np.asarray(active, dtype=bool)
    return float(np.asarray(ev, dtype=np.float64)[act].sum()) + float(dbl_score) + label_term(np.asarray(n_sing)[act], int(n_dbl))
