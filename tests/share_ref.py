"""numpy restatement of the continuous mixing share (dmx_engine_share_scan / dmx_engine_share_fit), shared by
tests/test_share_cpu.py and tests/test_gpu_share.py.

p_lm, q_lm and s_lm are formed in float64 exactly as include/dmx.h states (they are the kernels' inputs); everything after them runs in
long double and in logs: log f_lm = sum_r log t, S1 = sum_r u, S2 = sum_r u u, then per pair, scaled by the largest weighted entry,
L = sum w f, L' = sum w f s S1, L'' = sum w f ((s S1)^2 - s^2 S2), lg = log L, D1 = L' / L, D2 = L'' / L - D1^2.  Beside the three
sums an evaluation returns the magnitudes the rounding bounds of the GPU test are stated in:
  abs_lg = sum_i |lg_i|,  m1 = sum_i A1_i,  m2 = sum_i (A2_i + A1_i^2),   A1_i = sum_lm w f |s| sum_r|u| / L,
  A2_i = sum_lm w f ((|s| sum_r|u|)^2 + s^2 S2) / L.
`driver` restates the safeguarded Newton iteration step by step; `maximise` is the reference maximiser (bisection on LL' to 1e-12)."""
import numpy as np

from ambient_ref import host_pairs

LD = np.longdouble
INTERIOR, AT_0, AT_1, NOT_CONVERGED, FLAT, NONFINITE = 1, 2, 4, 8, 16, 32


class Evaluation:
    __slots__ = ("ll", "d1", "d2", "abs_lg", "m1", "m2", "n_snp", "n_read", "n_max")

    def values(self):
        """(LL, LL', LL'') rounded to float64."""
        return float(self.ll), float(self.d1), float(self.d2)


class ShareRef:
    def __init__(self, sp, g, mat, err, a=None, rho=None):
        self.po = np.asarray(sp.cell_pair_off, dtype=np.int64)
        _, self.snp, self.nrd, self.start = host_pairs(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd)
        self.reads = np.asarray(sp.reads)
        self.g = np.asarray(g, dtype=np.float32)
        self.mat, self.e3 = np.asarray(mat, dtype=np.float64), np.asarray(err, dtype=np.float64) / 3.0
        self.a = np.zeros(self.g.shape[0]) if a is None else np.asarray(a, dtype=np.float64)
        self.rho = np.zeros(len(self.po) - 1) if rho is None else np.asarray(rho, dtype=np.float64)

    def pair_terms(self, b, v1, v2, alpha):
        """(lg, D1, D2, A1, A2, nrd) per counted pair of barcode b in stored order, long double."""
        sl = slice(self.po[b], self.po[b + 1])
        snp, nrd, start = self.snp[sl], self.nrd[sl], self.start[sl]
        g1, g2 = self.g[snp, v1].astype(np.float64), self.g[snp, v2].astype(np.float64)
        ok = (nrd > 0) & (g1 != 0).any(axis=1) & (g2 != 0).any(axis=1)
        snp, nrd, start, g1, g2 = snp[ok], nrd[ok], start[ok], g1[ok], g2[ok]
        P = len(snp)
        rho, alpha = np.float64(self.rho[b]), np.float64(alpha)
        om = np.float64(1.0) - rho
        ra = rho * self.a[snp]                                                        # float64, as the header states
        c = np.array([0.5 * l + ((m - l) * 0.5) * alpha for l in range(3) for m in range(3)], dtype=np.float64)
        p = om * c[None, :] + ra[:, None]
        q = 1.0 - p
        s = np.array([(om * 0.5) * (m - l) for l in range(3) for m in range(3)], dtype=np.float64).astype(LD)
        pL, qL = p.astype(LD), q.astype(LD)
        logf = np.zeros((P, 9), dtype=LD)
        S1 = np.zeros((P, 9), dtype=LD)
        S1a = np.zeros((P, 9), dtype=LD)
        S2 = np.zeros((P, 9), dtype=LD)
        for r in range(int(nrd.max()) if P else 0):
            idx = np.flatnonzero(nrd > r)
            by = self.reads[start[idx] + r].astype(np.int64)
            bq, alt = by & 127, (by >> 7) != 0
            pR = np.where(alt, self.e3[bq], self.mat[bq]).astype(LD)[:, None]
            pA = np.where(alt, self.mat[bq], self.e3[bq]).astype(LD)[:, None]
            t = pR * qL[idx] + pA * pL[idx]
            with np.errstate(divide="ignore", invalid="ignore"):
                logf[idx] += np.log(t)
                u = np.where(t != 0, (pA - pR) / np.where(t != 0, t, 1), 0)
            S1[idx] += u
            S1a[idx] += np.abs(u)
            S2[idx] += u * u
        w = (g1[:, :, None] * g2[:, None, :]).reshape(P, 9).astype(LD)
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.where(w > 0, np.log(w) + logf, -np.inf)
            mx = x.max(axis=1, keepdims=True) if P else np.zeros((0, 1), dtype=LD)
            mf = np.where(np.isfinite(mx), mx, 0)
            T = np.exp(x - mf)
            L = T.sum(axis=1)
            sx, sxa = s[None, :] * S1, np.abs(s)[None, :] * S1a
            s2 = (s * s)[None, :] * S2
            lg = np.log(L) + mf[:, 0]
            D1 = (T * sx).sum(axis=1) / L
            D2 = (T * (sx * sx - s2)).sum(axis=1) / L - D1 * D1
            A1 = (T * sxa).sum(axis=1) / L
            A2 = (T * (sxa * sxa + s2)).sum(axis=1) / L
        return lg, D1, D2, A1, A2, nrd

    def evaluate(self, b, v1, v2, alpha) -> Evaluation:
        lg, D1, D2, A1, A2, nrd = self.pair_terms(b, v1, v2, alpha)
        e = Evaluation()
        z = LD(0)
        e.ll, e.d1, e.d2 = lg.sum() + z, D1.sum() + z, D2.sum() + z
        e.abs_lg, e.m1, e.m2 = float(np.abs(lg).sum()), float(A1.sum()), float((A2 + A1 * A1).sum())
        e.n_snp, e.n_read, e.n_max = len(lg), int(nrd.sum()), int(nrd.max()) if len(nrd) else 0
        return e


def driver(evalf, start=0.5, tol=1e-6, max_iter=30, near=None):
    """The iteration of dmx_engine_share_fit on evalf(alpha) -> (LL, LL', LL'') in float64.  Returns a dict of alpha, at (the values at
    alpha_hat), at0, at1, n_eval, status.  `near`, when a list, collects how close each branch decision was to its boundary."""
    def note(x):
        if near is not None:
            near.append(abs(float(x)))
    r0, r1 = evalf(0.0), evalf(1.0)
    n_eval, status = 2, 0
    fin = all(np.isfinite(v) for v in (*r0, *r1))
    if not fin:
        alpha, at, status = 0.0, r0, AT_0
    else:
        note(r0[1]); note(r1[1])
        dn0, up1 = r0[1] <= 0.0, r1[1] >= 0.0
        if dn0 and up1:
            note(r1[0] - r0[0])
            alpha, at, status = (1.0, r1, AT_1) if r1[0] > r0[0] else (0.0, r0, AT_0)
        elif dn0:
            alpha, at, status = 0.0, r0, AT_0
        elif up1:
            alpha, at, status = 1.0, r1, AT_1
        else:
            lo, hi, a, it = 0.0, 1.0, float(start), 0
            while True:
                r = evalf(a)
                n_eval += 1; it += 1
                if r[1] > 0.0:
                    lo = a
                else:
                    hi = a
                with np.errstate(divide="ignore", invalid="ignore"):
                    an = float(np.float64(a) - np.float64(r[1]) / np.float64(r[2]))
                note(r[2])
                if r[2] < 0.0:                # the step starts on the end just moved: it can leave the bracket at the other end,
                    note(hi - an if r[1] > 0.0 else an - lo)
                    if abs(an - a) <= 4.0 * np.spacing(a):       # ... or round onto its start
                        note(0.0)
                if not (r[2] < 0.0 and lo < an < hi):
                    an = (lo + hi) * 0.5
                note(abs(an - a) - tol)
                conv = abs(an - a) <= tol
                a = an
                if conv or it >= max_iter:
                    if not conv:
                        status |= NOT_CONVERGED
                    break
                note(r[1])                   # (the sign of LL' matters only when the bracket is used again)
            at = evalf(a)
            n_eval += 1
            alpha, status = a, status | INTERIOR
    if at[2] >= 0.0:
        status |= FLAT
    if not all(np.isfinite(v) for v in (*r0, *r1, *at)):
        status |= NONFINITE
    return dict(alpha=alpha, at=at, at0=r0, at1=r1, n_eval=n_eval, status=status)


def maximise(evalx, eps=1e-12):
    """The reference maximiser of a profile that rises at 0 and falls at 1: bisection on LL' in long double until hi - lo <= eps.
    evalx(alpha) -> Evaluation.  Returns (alpha*, Evaluation at alpha*)."""
    lo, hi = LD(0), LD(1)
    while hi - lo > eps:
        mid = (lo + hi) / 2
        if evalx(float(mid)).d1 > 0:
            lo = mid
        else:
            hi = mid
    a = float((lo + hi) / 2)
    return a, evalx(a)
