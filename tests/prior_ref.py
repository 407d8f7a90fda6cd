"""numpy restatement of the empirical-Bayes prior model, written from the model's statement and not from the
kernels: float64, or longdouble with longdouble=True.

For barcode b with L[j][k][n] = grid[b][j][k][n]: S_j = L[j][0][0]; D_jkn = L[j][k][n] for j != k, n >= 1; nothing else is used.
  w_S(j) = (1 - d) pi_j + d pi_j^2,  w_D(j,k,n) = d pi_j pi_k / (A - 1),
  E_b = sum_j w_S(j) exp(S_j) + sum_{j != k, n >= 1} w_D(j,k,n) exp(D_jkn),  LL = sum_b log E_b,
  r = w exp(.) / E_b,  h_j = r_S(j) d pi_j / ((1 - d) + d pi_j),
  N_j = sum_b [r_S(j) + h_j + sum_{k,n} r_D(j,k,n) + sum_{k,n} r_D(k,j,n)],  pi' = N / sum N,  d' = min(1, sum_b [sum_j h_j + sum r_D] / B_in).
A term of weight 0 or entry -inf is exactly 0.  A barcode is flagged MASKED (1) when mask[b] == 0 and BAD (2) with a NaN or +inf among
its used entries or without a term above zero; flagged barcodes get zeros and count nowhere."""
import numpy as np

MASKED, BAD = 1, 2
CHUNK = 64


def weights(pi, d, A, T=np.float64):
    """(pi / sum(pi), w_S[V], w_D[V][V] per alpha with a zero diagonal): they sum to 1 over j, (j != k) and the A - 1 alphas."""
    pi = np.asarray(pi, dtype=T)
    pi = pi / pi.sum()
    d = T(d)
    wS = (1 - d) * pi + d * pi * pi
    wD = d * pi[:, None] * pi[None, :] / T(A - 1)
    wD[np.diag_indices(len(pi))] = 0
    return pi, wS, wD


def _terms(grid, pi, d, mask, T):
    g = np.asarray(grid, dtype=np.float64)
    B, V, _, A = g.shape
    pi, wS, wD = weights(pi, d, A, T)
    d = T(d)
    with np.errstate(divide="ignore"):
        lpi = np.log(pi)
        lwS = np.log(wS)
        ld = np.log(d / T(A - 1)) if d > 0 else T(-np.inf)
        lwD = (ld + lpi[None, :]) + lpi[:, None]
    off = ~np.eye(V, dtype=bool)
    lwD = np.where(off & (wD > 0), lwD, -np.inf)
    S = g[:, :, 0, 0].astype(T)
    D = g[:, :, :, 1:].astype(T)
    bad = (~(S < np.inf)).any(axis=1) | (~(D < np.inf) & off[None, :, :, None]).any(axis=(1, 2, 3))
    with np.errstate(invalid="ignore"):
        xS = np.where((lwS > -np.inf)[None, :] & (S > -np.inf), S + lwS[None, :], -np.inf)
        xD = np.where((lwD > -np.inf)[None, :, :, None] & (D > -np.inf), D + lwD[None, :, :, None], -np.inf)
    m = np.maximum(xS.max(axis=1), xD.max(axis=(1, 2, 3)))
    bad |= ~(m > -np.inf)
    flags = np.where(bad, BAD, 0).astype(np.uint8)
    if mask is not None:
        flags[np.asarray(mask) == 0] = MASKED
    ok = flags == 0
    m = np.where(ok, m, 0)
    xS = np.where(ok[:, None], xS, -np.inf)
    xD = np.where(ok[:, None, None, None], xD, -np.inf)
    den = (1 - d) + d * pi
    with np.errstate(divide="ignore", invalid="ignore"):
        hf = np.where((wS > 0) & (den > 0), d * pi / np.where(den > 0, den, 1), 0)
    return dict(B=B, V=V, A=A, pi=pi, d=d, xS=xS, xD=xD, m=m, flags=flags, ok=ok, hf=hf)


def step(grid, pi, d, mask=None, longdouble=False):
    """One E + M.  Returns dict(N[V], hom, het, ll, b_in, pi_next[V], d_next, rows[B][V + 3], flags[B], log_e[B])."""
    T = np.longdouble if longdouble else np.float64
    t = _terms(grid, pi, d, mask, T)
    ok, m = t["ok"], t["m"]
    tS = np.exp(t["xS"] - m[:, None])
    tD = np.exp(t["xD"] - m[:, None, None, None])
    E = tS.sum(axis=1) + tD.sum(axis=(1, 2, 3))
    E1 = np.where(ok, E, 1)
    rS = tS / E1[:, None]
    rD = tD / E1[:, None, None, None]
    h = rS * t["hf"][None, :]
    Nb = rS + h + rD.sum(axis=(2, 3)) + rD.sum(axis=(1, 3))
    log_e = np.where(ok, m + np.log(E1), 0)
    rows = np.concatenate([Nb, h.sum(axis=1)[:, None], rD.sum(axis=(1, 2, 3))[:, None], log_e[:, None]], axis=1)
    rows = np.where(ok[:, None], rows, 0)
    V = t["V"]
    tot = rows[ok].sum(axis=0)
    b_in = int(ok.sum())
    N, hom, het, ll = tot[:V], tot[V], tot[V + 1], tot[V + 2]
    pi_next = N / N.sum() if b_in else t["pi"]
    d_next = min(T(1), (hom + het) / b_in) if b_in else t["d"]
    return dict(N=N, hom=hom, het=het, ll=ll, b_in=b_in, pi_next=pi_next, d_next=d_next, rows=rows, flags=t["flags"], log_e=log_e)


def fold_chunked(rows, flags):
    """The fold's float64 sum order: the included rows in ascending barcode id cut into chunks of 64, a chunk's rows added in order from
    0.0, the chunk partials added in ascending chunk order from 0.0."""
    inc = np.asarray(rows, dtype=np.float64)[np.asarray(flags) == 0]
    tot = np.zeros(inc.shape[1])
    for c0 in range(0, len(inc), CHUNK):
        part = np.zeros(inc.shape[1])
        for r in inc[c0:c0 + CHUNK]:
            part = part + r
        tot = tot + part
    return tot


def fit(grid, pi0=None, d0=0.1, max_iter=200, tol=1e-6, mask=None, fix_pi=False, fix_d=False, longdouble=False):
    """The EM loop: iteration t evaluates at (pi_t, d_t), records LL_t and d_t and moves to the M-step's image; it stops after the
    iteration whose LL_t - LL_{t-1} < tol * B_in (tol <= 0: never) or after max_iter; one more step at the final (pi, d) gives the
    reported N, hom, het, ll."""
    T = np.longdouble if longdouble else np.float64
    V = np.asarray(grid).shape[1]
    pi = np.full(V, 1.0, dtype=T) if pi0 is None else np.asarray(pi0, dtype=T)
    pi = pi / pi.sum()
    d = T(d0)
    lls, ds, conv = [], [], False
    for it in range(max_iter):
        s = step(grid, pi, d, mask, longdouble)
        if s["b_in"] == 0:
            raise ValueError("no barcode is included")
        lls.append(s["ll"]); ds.append(d)
        if not fix_pi:
            pi = s["pi_next"]
        if not fix_d:
            d = s["d_next"]
        if it > 0 and tol > 0 and lls[-1] - lls[-2] < tol * s["b_in"]:
            conv = True
            break
    s = step(grid, pi, d, mask, longdouble)
    return dict(pi=pi, d=d, ll=s["ll"], N=s["N"], hom=s["hom"], het=s["het"], b_in=s["b_in"], n_iter=len(lls), converged=conv,
                ll_trace=np.array(lls), d_trace=np.array(ds))


def call(grid, pi, d, mask=None, longdouble=False):
    """The per-barcode records at (pi, d): dict of arrays [B] log_e, p_sng, p_het, p_hom, p_sng1, p_sng2, p_dbl1, i_sng1, i_sng2, j_dbl,
    k_dbl, n_dbl, flag, plus xS[B][V] and xD[B][V][V][A - 1], the logarithms of the terms (-inf = a term that is zero), for a test's
    near-tie rule.  First maximum wins; the second singlet is the first maximum of the rest; the doublet is the first maximum in the
    order j, k, n ascending (-1 without a doublet term above zero)."""
    T = np.longdouble if longdouble else np.float64
    t = _terms(grid, pi, d, mask, T)
    s = step(grid, pi, d, mask, longdouble)
    B, V, A, ok, m = t["B"], t["V"], t["A"], t["ok"], t["m"]
    xS, xD = t["xS"], t["xD"]
    tS = np.exp(xS - m[:, None])
    tD = np.exp(xD - m[:, None, None, None])
    E = np.where(ok, tS.sum(axis=1) + tD.sum(axis=(1, 2, 3)), 1)
    rS = tS / E[:, None]
    i1 = np.full(B, -1); i2 = np.full(B, -1); jd = np.full(B, -1); kd = np.full(B, -1); nd = np.full(B, -1)
    p1 = np.zeros(B, dtype=T); p2 = np.zeros(B, dtype=T); pd1 = np.zeros(B, dtype=T)
    for b in np.flatnonzero(ok):
        a = int(np.argmax(xS[b]))
        rest = [j for j in range(V) if j != a]
        c = rest[int(np.argmax(xS[b][rest]))]
        i1[b], i2[b], p1[b], p2[b] = a, c, rS[b, a], rS[b, c]
        flat = xD[b].reshape(-1)
        f = int(np.argmax(flat))
        if flat[f] > -np.inf:
            jd[b], kd[b], nd[b] = f // (V * (A - 1)), (f // (A - 1)) % V, f % (A - 1) + 1
            pd1[b] = tD[b].reshape(-1)[f] / E[b]
    rows = s["rows"]
    p_hom, p_het = rows[:, V], rows[:, V + 1]
    h = rS * t["hf"][None, :]
    p_sng = np.where(ok, (rS - h).sum(axis=1), 0)
    return dict(log_e=s["log_e"], p_sng=p_sng, p_het=p_het, p_hom=p_hom, p_sng1=p1, p_sng2=p2, p_dbl1=pd1, i_sng1=i1, i_sng2=i2,
                j_dbl=jd, k_dbl=kd, n_dbl=nd, flag=t["flags"].astype(np.int32), xS=xS, xD=xD)
