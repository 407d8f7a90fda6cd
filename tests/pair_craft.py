"""Crafted barcodes for the `.pair` text tests (test_pair_craft_cpu.py, test_gpu_pair_text.py): K3's three scalars of a grid, and grids whose certified
entries (K3b: llksAB[a][b][n], llksAB[b][a][n] of an alpha = 0.5 best doublet) move one POSTPRB value across a 5-digit rounding boundary.

Why a certified entry can move a digit: POSTPRB = exp(v) * c / S with S = sum_i w_i exp(g_i) (maxLLK cancels).  The best doublet holds a share f of S, so
entries that are `delta` above the grid's raise S by f * delta (relative) and lower every other row's posterior by as much: 5e-12 (inside the STRICT bound of
7e-12) or 5e-11 (inside the FAST bound of 6e-11) against a device margin of 4e-13.  straddle_case() tunes one probe row, with mpmath at 60 digits, so that
the true scaled posterior lies >= 1e-12 (relative) on one side of a boundary with the certified entries and >= 1e-12 on the other side without them; every
other row is >= 1e-9 from every boundary under both, so no other field of the barcode may legitimately be left to the host."""
import math
from collections import namedtuple

import mpmath as mp
import numpy as np

mp.mp.dps = 60
PRIOR = 0.5
PROBE_MARGIN = 1e-12          # 2.5 x the device margin (4e-13); > 100 x any libm / device difference of a sum over 2 V^2 terms (~1e-16 each)
OTHER_MARGIN = 1e-9

Case = namedtuple("Case", "grid ovr probe V alphas delta sign")     # ovr = (a, b, n, llk_ab, llk_ba); probe = (j, k, a) with k == j, a == 0 for a singlet row


def rows_of(V, alphas):
    """(j, k, a) of a barcode's rows in print order (cmd_cram_demuxlet.cpp:772-797); singlet rows: k == j, a == 0."""
    out = []
    for j in range(V):
        out.append((j, j, 0))
        for k in range(V):
            for a in range(1, len(alphas)):
                if j == k or (j > k and alphas[a] == 0.5):
                    continue
                out.append((j, k, a))
    return out


def entry_of(row):
    j, k, a = row
    return (j, 0, 0) if a == 0 else (j, k, a)


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def k3_scalars(grid, alphas, prior=PRIOR):
    """max_llk, sum_single, sum_double of one barcode's grid [V][V][A]: call_cell's expression and serial order (dmx_host.cpp) with math.exp; the maximum starts
    at -1e300 and skips NaN, as `max < v` and the device's fmax do."""
    V, _, A = grid.shape
    mx = -1e300
    for v in grid.reshape(-1).tolist():
        if mx < v:
            mx = v
    g = grid.tolist()
    ss = sd = 0.0
    for j in range(V):
        ss += (_exp(g[j][0][0] - mx) * (1. - prior) / V)
        for k in range(V):
            if j == k:
                continue
            for a in range(1, A):
                sd += (_exp(g[j][k][a] - mx) * prior / V / (V - 1) / (A - 1) / (2.0 if alphas[a] == 0.5 else 1.0))
    return mx, ss, sd


def substituted(grid, ovr):
    """The grid the host formatter prints from: the two certified entries in place (dmx_host.cpp, the scratch grid of a certified barcode)."""
    g = grid.copy()
    if ovr is not None:
        a, b, n, v_ab, v_ba = ovr
        g[a, b, n] = v_ab
        g[b, a, n] = v_ba
    return g


def host_post(v, scal, V, A, singlet, prior=PRIOR):
    """The posterior of :780 / :792, operation by operation, on (max_llk, sum_single, sum_double)."""
    mx, ss, sd = scal
    tot = ss + sd
    e = _exp(v - mx)
    return e * (1. - prior) / V / tot if singlet else e * prior / V / (V - 1) / (A - 1) / tot


def _weights(V, alphas, prior):
    A = len(alphas)
    w = np.zeros((V, V, A))
    for j in range(V):
        w[j, 0, 0] = (1. - prior) / V
        for k in range(V):
            if j != k:
                for a in range(1, A):
                    w[j, k, a] += prior / V / (V - 1) / (A - 1) / (2.0 if alphas[a] == 0.5 else 1.0)
    return w


def true_sum(grid, alphas, shift, prior=PRIOR):
    """S * exp(-shift) at mp precision (the weights are small rationals; their double rounding, ~1e-16, is far below every margin used here)."""
    V = grid.shape[0]
    w = _weights(V, alphas, prior)
    s = mp.mpf(0)
    for idx in zip(*np.nonzero(w)):
        s += mp.mpf(float(w[idx])) * mp.exp(mp.mpf(float(grid[idx])) - shift)
    return s


def true_post(grid, alphas, row, S, shift, prior=PRIOR):
    V, A = grid.shape[0], len(alphas)
    v = mp.mpf(float(grid[entry_of(row)]))
    c = mp.mpf(1. - prior) / V if row[2] == 0 else mp.mpf(prior) / V / (V - 1) / (A - 1)
    return mp.exp(v - shift) * c / S


def boundary_distance(p):
    """(signed relative distance of the scaled posterior t in [1e4, 1e5) to the nearest 5-digit rounding boundary: (frac(t) - 0.5) / t, the boundary itself)."""
    X = int(mp.floor(mp.log10(p)))
    t = p * mp.mpf(10) ** (4 - X)
    fl = mp.floor(t)
    return (t - fl - mp.mpf("0.5")) / t, (fl + mp.mpf("0.5")) * mp.mpf(10) ** (X - 4)


def _ulps(x, n):
    for _ in range(abs(n)):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


def straddle_case(V, alphas, delta, sign, rng, singlet_probe):
    """A grid [V][V][A], an override and a probe row as the module docstring says.  sign = +1: certified entries above the grid's, -1: below."""
    A = len(alphas)
    halves = [a for a in range(1, A) if alphas[a] == 0.5]
    assert halves and V >= 3
    rows = rows_of(V, alphas)
    for _attempt in range(200):
        M = -float(rng.uniform(20.0, 200.0))
        grid = M - rng.uniform(8.0, 600.0, size=(V, V, A))                  # v - max in [-600, 0]; the best doublet keeps > 0.99 of the posterior
        a, b = sorted(int(x) for x in rng.choice(V, size=2, replace=False))
        n = int(rng.choice(halves))
        for h in halves:                                                        # (j, k) and (k, j) are one doublet at alpha = 0.5
            for j in range(V):
                for k in range(j):
                    grid[j, k, h] = grid[k, j, h]
        grid[a, b, n] = grid[b, a, n] = M
        cert = M + sign * delta
        ovr = (a, b, n, cert, cert)
        cand = [r for r in rows if (r[2] == 0) == singlet_probe and r != (a, b, n)]
        probe = cand[int(rng.integers(len(cand)))]
        pe = entry_of(probe)
        grid[pe] = M - float(rng.uniform(6.0, 30.0))
        if probe[2] in halves:
            grid[probe[1], probe[0], probe[2]] = grid[pe]
        shift = mp.mpf(M)
        ok = False
        for _round in range(40):
            gc = substituted(grid, ovr)
            Su, Sc = true_sum(grid, alphas, shift), true_sum(gc, alphas, shift)
            # ---- the probe: centre a boundary between the two variants' posteriors
            pu, pc = true_post(grid, alphas, probe, Su, shift), true_post(gc, alphas, probe, Sc, shift)
            mid = mp.sqrt(pu * pc)
            _, bnd = boundary_distance(mid)
            v0 = float(grid[pe]) + float(mp.log(bnd / mid))
            best = None
            for u in (0, 1, -1, 2, -2, 3, -3):                                  # a double next to the centre that leaves enough margin
                if best is not None and best[0] >= 1.5 * PROBE_MARGIN:
                    break
                g2 = grid.copy()
                g2[pe] = _ulps(v0, u)
                if probe[2] in halves:
                    g2[probe[1], probe[0], probe[2]] = g2[pe]
                g2c = substituted(g2, ovr)
                S2u, S2c = true_sum(g2, alphas, shift), true_sum(g2c, alphas, shift)
                du, _ = boundary_distance(true_post(g2, alphas, probe, S2u, shift))
                dc, _ = boundary_distance(true_post(g2c, alphas, probe, S2c, shift))
                if du * dc < 0 and (best is None or min(abs(du), abs(dc)) > best[0]):
                    best = (min(abs(du), abs(dc)), g2)
            if best is None or best[0] < PROBE_MARGIN:
                break                                                           # share of the best doublet too small for this delta: draw again
            grid = best[1]
            # ---- every other row: >= 1e-9 from every boundary under both variants, else draw it again (which moves S: go round once more)
            gc = substituted(grid, ovr)
            Su, Sc = true_sum(grid, alphas, shift), true_sum(gc, alphas, shift)
            redrawn = False
            for r in rows:
                if r == probe:
                    continue
                d1, _ = boundary_distance(true_post(gc, alphas, r, Sc, shift))
                d2, _ = boundary_distance(true_post(gc, alphas, r, Su, shift))   # the certified value on the record's sums: what the device printed before
                if min(abs(d1), abs(d2)) >= OTHER_MARGIN:
                    continue
                if r == (a, b, n):
                    redrawn = None
                    break
                e = entry_of(r)
                grid[e] = M - float(rng.uniform(8.0, 600.0))
                if r[2] in halves:
                    grid[r[1], r[0], r[2]] = grid[e]
                redrawn = True
            if redrawn is None:
                break
            if not redrawn:
                ok = True
                break
        if ok:
            return Case(grid, ovr, probe, V, tuple(alphas), delta, sign)
    raise RuntimeError("straddle_case: no grid found")


_cache = {}


def straddle_cases(V, alphas, reps=1, seed=0):
    """reps x (delta in 5e-12, 5e-11) x (sign +, -) x (singlet probe, doublet probe), built once per (V, alphas, reps, seed)."""
    key = (V, tuple(alphas), reps, seed)
    if key not in _cache:
        rng = np.random.default_rng([seed, V, len(alphas)])
        _cache[key] = [straddle_case(V, alphas, delta, sign, rng, sp)
                       for _ in range(reps) for delta in (5e-12, 5e-11) for sign in (+1, -1) for sp in (True, False)]
    return _cache[key]


def check_case(case):
    """The distances straddle_case promises, recomputed from the returned grid alone: (probe distance certified, probe distance uncertified, smallest distance
    of any other row under either set of sums)."""
    grid, ovr, probe, V, alphas = case.grid, case.ovr, case.probe, case.V, case.alphas
    gc = substituted(grid, ovr)
    shift = mp.mpf(float(grid[ovr[0], ovr[1], ovr[2]]))
    Su, Sc = true_sum(grid, alphas, shift), true_sum(gc, alphas, shift)
    dc, _ = boundary_distance(true_post(gc, alphas, probe, Sc, shift))
    du, _ = boundary_distance(true_post(grid, alphas, probe, Su, shift))
    other = min(min(abs(boundary_distance(true_post(gc, alphas, r, S, shift))[0]) for S in (Sc, Su)) for r in rows_of(V, alphas) if r != probe)
    return dc, du, other
