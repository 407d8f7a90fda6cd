"""float64 numpy restatement of the census uncertainty (Engine.census_fisher, census.covariance, the presence test).

At shares w the quotients tR = pR / P_r, tA = pA / P_r of a stored read are formed with census_ref.step's operations (the device's), and
so are the per-pair sums sR, sA, sRR = sum tR tR, sRA = sum tR tA, sAA = sum tA tA (np.bincount adds in stored order).  With e = 1 - d,
  H[v][u]     = sum over pairs of ((e_v e_u) sRR + (e_v d_u + d_v e_u) sRA) + (d_v d_u) sAA,
  score[b][v] = sum over the pairs of barcode b of e_v sR + d_v sA,
each term in float64 with the operations in that order, the sums over pairs in extended precision (the device's order is its own,
include/dmx.h).  H is formed a few rows at a time, so V = 128 needs megabytes.  Also here: an independent statement of the two
covariances, the census driver with the gap on the start's support, the presence test on it, and a pool whose barcodes each hold one
donor's reads."""
import math
from dataclasses import dataclass

import numpy as np

import census_ref as R

U = R.U


@dataclass
class Fisher:
    H: np.ndarray            # [V][V]
    score: np.ndarray        # [B][V], zero rows for barcodes outside the group
    n_read_b: np.ndarray     # [B]
    n_pair_b: np.ndarray     # [B]
    acc: np.ndarray          # [V] = the sum of the score rows, in extended precision
    n_read: int
    n_pair: int


def pair_sums(fl: R.Flat, d, valid, member, w, mat, err):
    """(use[P], sR, sA, sRR, sRA, sAA over the used pairs)."""
    w = np.asarray(w, dtype=np.float64)
    use = np.asarray(member, dtype=bool)[fl.cell] & (fl.nrd > 0) & valid[fl.snp]
    ru = use[fl.read_pair]
    rp = fl.read_pair[ru]
    tR, tA = R.phred(mat, err)
    pR, pA = tR[fl.byte[ru]], tA[fl.byte[ru]]
    A = R.ambient_profile(w, d)[fl.snp[rp]]
    with np.errstate(all="ignore"):
        P = pR * (1.0 - A) + pA * A
        qR, qA = pR / P, pA / P
    n = len(fl.cell)
    out = [np.bincount(rp, weights=x, minlength=n)[use] for x in (qR, qA, qR * qR, qR * qA, qA * qA)]
    return (use, *out)


def fisher(fl: R.Flat, d, valid, member, w, mat, err, rows=4, only=None) -> Fisher:
    """`only`: the rows of H to form (the others are NaN); everything else is always whole."""
    V = d.shape[1]
    use, sR, sA, sRR, sRA, sAA = pair_sums(fl, d, valid, member, w, mat, err)
    B = fl.n_cells
    cell = fl.cell[use]
    dd = d[fl.snp[use]]
    ee = 1.0 - dd
    H = np.zeros((V, V)) if only is None else np.full((V, V), np.nan)
    want = np.arange(V) if only is None else np.asarray(only, dtype=np.int64)
    for i in range(0, len(want), rows):
        r = want[i:i + rows]
        dv, ev = dd[:, r, None], ee[:, r, None]
        du, eu = dd[:, None, :], ee[:, None, :]
        t = ((ev * eu) * sRR[:, None, None] + (ev * du + dv * eu) * sRA[:, None, None]) + (dv * du) * sAA[:, None, None]
        H[r] = t.sum(axis=0, dtype=np.longdouble).astype(np.float64)
    terms = (ee * sR[:, None] + dd * sA[:, None]).astype(np.longdouble)
    score = np.zeros((B, V), dtype=np.longdouble)
    np.add.at(score, cell, terms)
    n_read_b = np.bincount(cell, weights=fl.nrd[use], minlength=B).astype(np.int64)
    n_pair_b = np.bincount(cell, minlength=B).astype(np.int64)
    return Fisher(H, score.astype(np.float64), n_read_b, n_pair_b, score.sum(axis=0).astype(np.float64), int(n_read_b.sum()), int(use.sum()))


def fisher_brute(fl: R.Flat, d, valid, member, w, mat, err, dtype=np.float64):
    """H = sum over reads of f_r f_r' / P_r^2, f_rv = pR (1 - d_v) + pA d_v, P_r = sum_v w_v f_rv, in `dtype`."""
    use = np.asarray(member, dtype=bool)[fl.cell] & (fl.nrd > 0) & valid[fl.snp]
    ru = use[fl.read_pair]
    rp = fl.read_pair[ru]
    tR, tA = R.phred(mat, err)
    pR, pA = tR[fl.byte[ru]].astype(dtype)[:, None], tA[fl.byte[ru]].astype(dtype)[:, None]
    dr = d[fl.snp[rp]].astype(dtype)
    f = pR * (1 - dr) + pA * dr
    P = f @ np.asarray(w).astype(dtype)
    q = f / P[:, None]
    return q.T @ q


def covariance(H, w, n_read, score, n_b, min_reads=1.0):
    """(se, se_robust, at_bound) stated independently of census.covariance: the free shares are parametrised by all but the last free
    donor (the last takes what is left), the information and the barcodes' scores are carried to that chart, inverted there and carried
    back.  The result does not depend on the chart.  NaN where census.covariance says NA."""
    H, w = np.asarray(H, dtype=np.float64), np.asarray(w, dtype=np.float64)
    V = len(w)
    at_bound = ~(w * float(n_read) > min_reads)
    F = np.flatnonzero(~at_bound)
    f = len(F)
    se, se_r = np.zeros(V), np.zeros(V)
    if f < 2:
        return se, se_r, at_bound
    T = np.vstack([np.eye(f - 1), -np.ones((1, f - 1))])            # d w_F / d theta
    G1 = T.T @ H[np.ix_(F, F)] @ T
    if not np.isfinite(G1).all() or np.linalg.cond(G1) > 1e11:
        se[F] = se_r[F] = np.nan
        return se, se_r, at_bound
    Gi = np.linalg.inv(G1)
    se[F] = np.sqrt(np.maximum(np.diag(T @ Gi @ T.T), 0.0))
    used = np.asarray(n_b) > 0
    Bg = int(used.sum())
    if Bg < 2 * f:
        se_r[F] = np.nan
    else:
        s = (np.asarray(score)[used][:, F] - np.asarray(n_b, dtype=np.float64)[used][:, None]) @ T
        se_r[F] = np.sqrt(np.maximum(np.diag(T @ Gi @ (s.T @ s) @ Gi @ T.T) * Bg / (Bg - 1.0), 0.0))
    return se, se_r, at_bound


def run(fl: R.Flat, d, valid, member, mat, err, w0=None, tol=1e-4, max_steps=2000, accelerate=True, gap_on_support=False):
    """census_ref.run with include/dmx.h's gap_on_support: the gap's maximum runs over the donors with w0 > 0."""
    V = d.shape[1]
    x = np.full(V, 1.0 / V) if w0 is None else np.asarray(w0, dtype=np.float64).copy()
    support = x > 0.0
    phase, steps = 0, 0
    a0 = a1 = a2 = None
    ll1 = 0.0
    while True:
        s = R.step(fl, d, valid, member, x, mat, err)
        steps += 1
        empty = s.n_read == 0
        gap = s.gap
        if gap_on_support and not empty:
            gap = s.n_read * (max(0.0, float(s.acc[support].max())) / s.n_read - 1.0)
        conv = empty or (math.isfinite(s.ll) and gap <= tol)
        if conv or steps >= max_steps:
            return dict(w=x, ll=0.0 if empty else s.ll, gap=0.0 if empty else gap, n_steps=steps, converged=int(conv), n_read=s.n_read,
                        n_pair=s.n_pair)
        if not accelerate:
            x = R.em_image(x, s)
        elif phase == 0:
            a0, a1 = x, R.em_image(x, s)
            x, phase = a1, 1
        elif phase == 1:
            ll1, a2 = s.ll, R.em_image(x, s)
            x, phase = R.extrapolate(a0, a1, a2), 2
        else:
            x = a2 if (not math.isfinite(s.ll) or s.ll < ll1) else R.em_image(x, s)
            phase = 0


def presence(fl: R.Flat, d, valid, member, mat, err, full, tol=1e-4, max_steps=2000, gap_on_support=True, min_reads=1.0, donors=None):
    """The presence test of one group from its fit `full` (a run() result): per donor dict(llr, p, n_steps, converged).  The donors at
    the bound (w N <= min_reads) get LLR 0 and P 1 and stay at 0 in the refits of the others."""
    w = full["w"]
    bound = ~(w * full["n_read"] > min_reads)
    out = {}
    for v in (range(len(w)) if donors is None else donors):
        if bound[v]:
            out[v] = dict(llr=0.0, p=1.0, n_steps=0, converged=1)
            continue
        x = np.where(bound, 0.0, w)
        x[v] = 0.0
        x = x / x.sum()
        x = x / x.sum()
        r = run(fl, d, valid, member, mat, err, w0=x, tol=tol, max_steps=max_steps, gap_on_support=gap_on_support)
        llr = max(full["ll"] - r["ll"], 0.0)
        out[v] = dict(llr=llr, p=0.5 * math.erfc(math.sqrt(llr)), n_steps=r["n_steps"], converged=r["converged"], w=r["w"])
    return out


def make_cell_pool(rng, alleles, shares, B, n_reads, bq_lo=10, bq_hi=40):
    """A pool whose barcodes each hold ONE donor's reads (a group of cells): every barcode draws its donor from `shares`, then reads
    are drawn as census_ref.make_pool draws them, the donor being the barcode's."""
    S, V = alleles.shape[:2]
    owner = rng.choice(V, B, p=np.asarray(shares) / np.sum(shares))
    cell = rng.integers(0, B, n_reads)
    snp = rng.integers(0, S, n_reads)
    al = np.clip(alleles[snp, owner[cell], rng.integers(0, 2, n_reads)], 0, 1)
    bq = rng.integers(bq_lo, bq_hi + 1, n_reads)
    wrong = rng.random(n_reads) < 10.0 ** (-bq / 10.0)
    other = rng.random(n_reads) < 1.0 / 3.0
    keep = ~wrong | other
    al = np.where(wrong, 1 - al, al)
    return R.build_pileup(B, S, cell[keep], snp[keep], ((al[keep] << 7) | bq[keep]).astype(np.uint8)), owner
