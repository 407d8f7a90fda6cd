"""CPU: the host emulator of the feature passes' contracts (tests/contract_emul.cpp) is right before any kernel is judged by it.

On the inputs of tests/test_gpu_contract_bits.py (tests/contract_emul.py) the emulator is compared with the float64 numpy restatements
the tolerance tests use (ambient_ref, ambient_dbl_ref, fit_ref, share_ref, site_ref, ref_refine / pair_gl of test_gpu_refine, ref_stage /
ref_mstep of test_gpu_cluster) within those tests' own tolerances, counts exactly; on one problem of test_mpmath_kat's size (50 barcodes x 120 SNPs x
4 samples) with 50-digit arithmetic written from include/dmx.h's formulas, at that file's 1e-12.  Three deliberately wrong variants of the
emulator (products contracted into FMAs, descending order, libm's log) must each change bits of every pass on these inputs, and the
emulator's counters state the conditions the GPU comparison rests on: no subnormal / inf / nan log argument anywhere, zero arguments only
in the case built for them, rescales taken in the deep cases of both ambient passes, n_trunc and n_zero reached by the goodness of fit,
every depth regime of quality_mix.DEPTHS present.  No GPU compute is called.

Measured against 50-digit arithmetic (max |delta|, printed by test_against_50_digit_arithmetic): ambient LL 4.3e-14,
ambient doublet LL 4.3e-14, fit obs 1.1e-13 / mean 2.1e-14 / var 1.8e-13, refinement LL 2.8e-14, cluster lgl 1.8e-15, M-step LL 2.1e-14 / W
2.7e-15; share scan LL 4.0e-14, share fit LL 3.9e-14, site obs 1.4e-14 / mean 7.1e-15 / var 2.9e-13 / exc 3.6e-15 / vexc 8.9e-15: every pass holds
1e-12.  LL' and LL'' of the share passes grow like 1 / err and are held to test_gpu_share's U k1 m1 and U k2 m2 with m1, m2, N and n_max
from the 50-digit run (max |delta| 1.4e-12 and 1.6e-9: at most 0.034 and 0.008 of the bounds).

The share scan, the share fit and the site audit (emu_share_scan, emu_share_fit, emu_site_fit) are compared with tests/share_ref.py and
tests/site_ref.py within the tolerances of test_gpu_share and test_site_cpu, and the conditions their GPU comparison rests on are
asserted on the emulator's own results: every status bit and every way out of the driver occurs, Newton steps are refused, interior
maxima are reached after three or more evaluations, both lists of the site audit take every length 0, 1, 63, 64, 65 and 129."""
import mpmath
import numpy as np
import pytest

import ambient_dbl_ref
import ambient_ref
import contract_emul as CE
import fit_ref
import quality_mix as QM
import share_ref
import site_ref
import test_gpu_cluster as TC
import test_gpu_refine as TR
import test_gpu_share as TS

TOL_MP = 1e-12          # test_mpmath_kat.TOL
TOL = 1e-9              # test_gpu_ambient / test_gpu_ambient_dbl / test_gpu_refine / test_gpu_cluster (LL)


@pytest.fixture(scope="module")
def m(tmp_path_factory):
    from demuxlet_amd import build, capi, engine, synth
    build.build()
    capi.load()
    d = tmp_path_factory.mktemp("contract_emul")
    mat, err = engine.phred_tables()
    return dict(engine=engine, synth=synth, emu=CE.build(d), fast=CE.build(d, contract=True), P=CE.problems(engine, synth), mat=mat, err=err,
                cache={})


def tables(m, p):
    return p.tables if p.tables is not None else (m["mat"], m["err"])


def same_or_close(x, y, tol, rel=False):
    """max |x - y| (over max(1, |y|) when rel) where y is finite; x must equal y where it is not."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    fin = np.isfinite(y)
    assert np.array_equal(x[~fin], y[~fin])
    if not fin.any():
        return 0.0
    d = np.abs(x[fin] - y[fin])
    if rel:
        d = d / np.maximum(1.0, np.abs(y[fin]))
    d = float(d.max())
    assert d <= tol, d
    return d


# ---- one run of a pass on a case, by emulator and variant (cached: the tests below share them) ---------------------------------------------

def run_ambient(m, emu, case):
    name, Q = case
    p = m["P"][name]
    return emu.ambient(p.sp, p.g, *tables(m, p), CE.assignment(p), CE.amb_freq(p), CE.GRIDS[Q])


def run_ambient_dbl(m, emu, case):
    name, Cn, A, Q = case
    p = m["P"][name]
    return emu.ambient_doublet(p.sp, p.g, *tables(m, p), CE.candidates(p, Cn), CE.ALPHAS[A], CE.amb_freq(p), CE.GRIDS[Q])


def run_fit(m, emu, case):
    name, M, soup = case
    p = m["P"][name]
    hyp, alpha, rho = CE.hypotheses(p)
    out, cnt = emu.fit(p.sp, p.g, *tables(m, p), hyp, alpha, rho if soup else None, CE.amb_freq(p) if soup else None, M)
    return tuple(out[k] for k in ("obs", "mean", "var", "n_snp", "n_read", "n_trunc", "n_zero")) + (cnt,)


def run_refine(m, emu, name):
    p = m["P"][name]
    return emu.refine(p.sp, p.g.shape[0], p.V, *tables(m, p), CE.refine_assignment(p))


def run_cluster(m, emu, case):
    """The stage of the problem and, where the case names a column count, the M-step over it."""
    name, Cn = case
    p = m["P"][name]
    off, cell, lgl, ra, cnt = emu.cluster_stage(p.sp, *tables(m, p))
    if Cn is None:
        return off, cell, lgl, ra, cnt
    LL, W = emu.cluster_mstep(off, cell, lgl, CE.mstep_weights(p, Cn))
    return off, cell, lgl, ra, LL, W, cnt


def soup(p, given):
    """(rho[B], a[S]) of a case, or (None, None)."""
    return (CE.barcode_rho(p), CE.amb_freq(p)) if given else (None, None)


def run_share_scan(m, emu, case):
    name, T, given = case
    p = m["P"][name]
    return emu.share_scan(p.sp, p.g, *tables(m, p), CE.anchors(p, T), *soup(p, given))


def run_share_fit(m, emu, case):
    name, Cn, start, tol, max_iter, probe, given = case
    p = m["P"][name]
    val, cts, _, cnt = emu.share_fit(p.sp, p.g, *tables(m, p), CE.share_candidates(p, Cn), *soup(p, given), start, tol, max_iter, probe)
    return val, cts, cnt


def site_arguments(p, case):
    """(hyp, alpha, rho or None, a or None, M) of a site case."""
    _, M, given, lists = case
    hyp, alpha, rho = CE.site_hypotheses(p, lists)
    return hyp, alpha, rho if given else None, CE.amb_freq(p) if given else None, M


def run_site_fit(m, emu, case):
    p = m["P"][case[0]]
    out, cnt = emu.site_fit(p.sp, p.g, *tables(m, p), *site_arguments(p, case))
    return tuple(out[k] for k in CE.SITE_FLOATS + CE.SITE_COUNTS) + (cnt,)


CLUSTER_CASES = [(n, None) for n in CE.REFINE_CASES] + CE.MSTEP_CASES
PASSES = {"ambient": (run_ambient, CE.AMBIENT_CASES), "ambient_doublet": (run_ambient_dbl, CE.AMBIENT_DBL_CASES), "fit": (run_fit, CE.FIT_CASES),
          "refine": (run_refine, CE.REFINE_CASES), "cluster": (run_cluster, CLUSTER_CASES), "share_scan": (run_share_scan, CE.SHARE_SCAN_CASES),
          "share_fit": (run_share_fit, CE.SHARE_FIT_CASES), "site_fit": (run_site_fit, CE.SITE_CASES)}


def result(m, pas, case, which="emu", variant=0):
    key = (pas, case, which, variant)
    if key not in m["cache"]:
        emu = m[which]
        emu.variant(variant)
        try:
            m["cache"][key] = PASSES[pas][0](m, emu, case)
        finally:
            emu.variant(0)
    return m["cache"][key]


# ---- against the float64 restatements -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CE.AMBIENT_CASES, ids=lambda c: f"{c[0]}-Q{c[1]}")
def test_ambient_against_restatement(m, case):
    p = m["P"][case[0]]
    ll, n_snp, n_read, _ = result(m, "ambient", case)
    sp = p.sp
    LL, ns, nr = ambient_ref.ref_profile(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, CE.assignment(p), p.g, CE.amb_freq(p),
                                         CE.GRIDS[case[1]], *tables(m, p))
    assert np.array_equal(n_snp, ns) and np.array_equal(n_read, nr)
    print(f"ambient {case}: max |delta| = {same_or_close(ll, LL, TOL):.2e} (|LL| up to {np.abs(LL[np.isfinite(LL)]).max(initial=0):.0f})")


@pytest.mark.parametrize("case", CE.AMBIENT_DBL_CASES, ids=lambda c: f"{c[0]}-C{c[1]}-A{c[2]}-Q{c[3]}")
def test_ambient_doublet_against_restatement(m, case):
    name, Cn, A, Q = case
    p = m["P"][name]
    ll, n_snp, n_read, _ = result(m, "ambient_doublet", case)
    sp = p.sp
    LL, ns, nr = ambient_dbl_ref.ref_dbl_profile(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, CE.candidates(p, Cn), p.g, CE.amb_freq(p),
                                                 CE.ALPHAS[A], CE.GRIDS[Q], *tables(m, p))
    assert np.array_equal(n_snp, ns) and np.array_equal(n_read, nr)
    print(f"ambient doublet {case}: max |delta| = {same_or_close(ll, LL, TOL):.2e}")


@pytest.mark.parametrize("case", CE.FIT_CASES, ids=lambda c: f"{c[0]}-M{c[1]}-{'soup' if c[2] else 'clean'}")
def test_fit_against_restatement(m, case):
    name, M, soup = case
    p = m["P"][name]
    out = dict(zip(("obs", "mean", "var", "n_snp", "n_read", "n_trunc", "n_zero"), result(m, "fit", case)))
    hyp, alpha, rho = CE.hypotheses(p)
    sp = p.sp
    mat, err = tables(m, p)
    args = (sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, hyp, alpha, rho if soup else None, CE.amb_freq(p) if soup else None, p.g, M, mat, err)
    r64, rld = fit_ref.ref_fit(*args), fit_ref.ref_fit(*args, longdouble=True)
    tol = fit_ref.tolerance(r64, rld)
    for k in ("n_snp", "n_read", "n_trunc", "n_zero"):
        assert np.array_equal(out[k], r64[k]), k
    for k in ("obs", "mean", "var"):
        d = fit_ref.scaled_difference(out[k], r64[k])
        assert d <= tol, (k, d, tol)


@pytest.mark.parametrize("name", CE.REFINE_CASES)
def test_refine_against_restatement(m, name):
    p = m["P"][name]
    ll, n_cell, n_ref, n_alt, _ = result(m, "refine", name)
    cell, snp, nrd, start = TR.host_pairs(p.sp)
    LL, nc, nr, na = TR.ref_refine(cell, snp, nrd, start, np.asarray(p.sp.reads), CE.refine_assignment(p), p.g.shape[0], p.V, *tables(m, p))
    assert np.array_equal(n_cell, nc) and np.array_equal(n_ref, nr) and np.array_equal(n_alt, na)
    same_or_close(ll, LL, TOL)
    if name.startswith("slab_"):
        sizes = np.bincount(CE.refine_assignment(p)[CE.refine_assignment(p) >= 0], minlength=p.V)
        assert sizes.tolist() == [0, 1, 63, 64, 65, 130]


@pytest.mark.parametrize("case", CLUSTER_CASES, ids=lambda c: f"{c[0]}-C{c[1]}")
def test_cluster_against_restatement(m, case):
    name, Cn = case
    p = m["P"][name]
    res = result(m, "cluster", case)
    off, cell, lgl, ra = res[:4]
    if p.tables is None:
        roff, rcell, rlgl, rref, ralt = TC.ref_stage(m, p.sp)
        assert np.array_equal(off, roff) and np.array_equal(cell, rcell)
        assert np.array_equal(ra & 0xFFFF, rref) and np.array_equal(ra >> 16, ralt)
        assert (np.abs(lgl - rlgl) <= 1e-12 * np.maximum(np.abs(rlgl), 1.0)).all(), np.abs(lgl - rlgl).max()
    if Cn is not None:
        LL, W = res[4:6]
        w = CE.mstep_weights(p, Cn)
        RL, RW, _ = TC.ref_mstep(off, cell, lgl, w, np.full((len(off) - 1, 3), 1 / 3, dtype=np.float32), 1e-3)
        assert np.abs(LL - RL).max() <= TOL
        assert (np.abs(W - RW) <= 1e-12 * np.maximum(np.abs(RW), 1.0)).all()
        n_slot = np.diff(off)
        if name.startswith("slab_"):
            assert (n_slot == 0).any() and (n_slot == 1).any()
        if w.size >= 100:
            assert (w == 0).any() and (w == 1).any() and (w == 1e-300).any()


class ShareBounds(TS.Shares):
    """test_gpu_share's check with its three bounds, and the one term its LL bound leaves out by its own account: the log's argument L
    carries 4 n + 10 roundings, which the log passes on as an absolute error of (4 n + 10) U per pair.  That file's pairs hold at most
    20 reads next to sum|lg| of hundreds; here a barcode may be ONE pair of 300 reads with |lg| = 0.1, where the left-out term is the
    whole error (measured 1.9e-16 against 1.3e-16 of the form without it).  LL' and LL'' keep U k1 m1 and U k2 m2 unchanged."""

    def check(self, got, ev, where):
        bll, b1, b2 = TS.bounds(ev)
        bll += TS.U * (4 * ev.n_max + 10) * ev.n_snp
        ref = ev.values()
        if not np.isfinite(ref[0]):
            assert not np.isfinite(got[0]) or got[0] == ref[0], where
            return
        d = [abs(float(np.longdouble(got[i]) - x)) for i, x in enumerate((ev.ll, ev.d1, ev.d2))]
        for k, dk, bk in (("ll" if ev.n_snp >= 63 else "ll_small", d[0], bll), ("d1", d[1], b1), ("d2", d[2], b2)):
            if bk > 0:
                self.s[k] = max(self.s[k], dk / bk)
            assert dk <= bk, (where, k, dk, bk)


# the barcodes a share case is compared on: those of the exact pair counts and every fifth of the rest (test_gpu_share's rule)
def share_barcodes(p):
    B = p.sp.n_cells
    return list(range(min(B, 12))) + list(range(12, B, 5))


@pytest.mark.parametrize("case", CE.SHARE_SCAN_CASES, ids=lambda c: f"{c[0]}-T{c[1]}-{'soup' if c[2] else 'clean'}")
def test_share_scan_against_restatement(m, case):
    """LL / LL' / LL'' within test_gpu_share's bounds of the long double restatement; the counts exactly."""
    name, T, given = case
    p = m["P"][name]
    out, nsr, _ = result(m, "share_scan", case)
    an = CE.anchors(p, T)
    rho, a = soup(p, given)
    ref = share_ref.ShareRef(p.sp, p.g, *tables(m, p), a, rho)
    sh = ShareBounds()
    V = p.V
    for b in range(p.sp.n_cells):
        sl = slice(p.sp.cell_pair_off[b], p.sp.cell_pair_off[b + 1])
        for t in range(T):
            v1 = int(an[b, t])
            if v1 < 0:
                assert not out[b, t].any() and not nsr[b, t].any()
                continue
            assert not out[b, t, v1].any()
            ok = (ref.nrd[sl] > 0) & (p.g[ref.snp[sl], v1] != 0).any(axis=1)
            assert nsr[b, t, 0] == ok.sum() and nsr[b, t, 1] == ref.nrd[sl][ok].sum()
            if b in share_barcodes(p):
                for v in [x for x in {(v1 + 1) % V, (v1 + V - 1) % V, (v1 + 31) % V, V - 1} if x != v1]:
                    sh.check(out[b, t, v], ref.evaluate(b, v1, v, 0.0), (b, t, v))
    sh.report(f"share scan {case}")


@pytest.mark.parametrize("case", CE.SHARE_FIT_CASES, ids=CE.share_fit_id)
def test_share_fit_against_restatement(m, case):
    """The four evaluations within test_gpu_share's bounds of the long double restatement; status and n_eval equal the restated driver's
    unless one of its decisions was within 1e-9 of its boundary (that test's rule, at most 2 % of the slots over all cases)."""
    name, Cn, start, tol, max_iter, probe, given = case
    p = m["P"][name]
    val, cts, _ = result(m, "share_fit", case)
    cand = CE.share_candidates(p, Cn)
    rho, a = soup(p, given)
    ref = share_ref.ShareRef(p.sp, p.g, *tables(m, p), a, rho)
    sh = ShareBounds()
    used = cand[:, :, 0] >= 0
    assert not val[~used].any() and not cts[~used].any()
    tally = m["cache"].setdefault("share_fit_tally", {})
    n_case = n_near = 0
    for b in share_barcodes(p):
        for c in [c for c in range(Cn) if used[b, c]][:2]:
            v1, v2 = (int(x) for x in cand[b, c])
            evs = {}

            def ev(x):
                if x not in evs:
                    evs[x] = ref.evaluate(b, v1, v2, x)
                return evs[x]
            near = []
            d = share_ref.driver(lambda x: ev(x).values(), start, tol, max_iter, near=near)
            n_case += 1
            e0 = ev(0.0)
            assert (cts[b, c, 2], cts[b, c, 3]) == (e0.n_snp, e0.n_read)
            al = float(val[b, c, 0])
            for o, x in ((4, 0.0), (7, 1.0), (1, al)) + (((10, probe),) if probe >= 0 else ()):
                sh.check(val[b, c, o:o + 3], ev(x), (b, c, x))
            if probe < 0:
                assert not val[b, c, 10:].any()
            exact = e0.m1 == 0.0 and ev(1.0).m1 == 0.0           # LL' = LL'' = +0 on both sides: decided without rounding
            if near and min(near) <= 1e-9 and not exact:
                n_near += 1
            else:
                assert cts[b, c, 1] == d["status"] and cts[b, c, 0] == d["n_eval"], (b, c, cts[b, c], d["status"], d["n_eval"])
                assert abs(al - d["alpha"]) <= 1e-9
    tally[case] = (n_case, n_near)
    sh.report(f"share fit {case}: {n_case} slots, {n_near} within 1e-9 of a branch boundary;")
    if len(tally) == len(CE.SHARE_FIT_CASES):
        assert sum(v[1] for v in tally.values()) <= 0.02 * sum(v[0] for v in tally.values()), tally


@pytest.mark.parametrize("case", CE.SITE_CASES, ids=CE.site_id)
def test_site_fit_against_restatement(m, case):
    """The ten arrays against site_ref.ref_site: counts exactly, floats within test_site_cpu's bound of ten times the restatement's own
    float64-to-long-double drift."""
    p = m["P"][case[0]]
    out = dict(zip(CE.SITE_FLOATS + CE.SITE_COUNTS, result(m, "site_fit", case)))
    hyp, alpha, rho, a, M = site_arguments(p, case)
    sp = p.sp
    args = (sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, hyp, alpha, rho, a, p.g, M, *tables(m, p))
    r64, rld = site_ref.ref_site(*args), site_ref.ref_site(*args, longdouble=True)
    tol = 10 * max(site_ref.drift(r64, rld), 1e-15)
    for k in CE.SITE_COUNTS:
        assert np.array_equal(out[k], r64[k]), k
    for k in CE.SITE_FLOATS:
        d = site_ref.scaled_difference(out[k], r64[k])
        assert d <= tol, (k, d, tol)


def same_bits_or_nan(x, y):
    """equal bits, or NaN on both sides (x86 and the device give 0 / 0 different signs and payloads; here both sides are one machine's)"""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and bool(((CE.bits(x) == CE.bits(y)) | (np.isnan(x) & np.isnan(y))).all())


IDENTITY_CASES = [c for c in CE.SHARE_FIT_CASES if c[0] in ("pool_02", "mix_full", "mix_edges", "panel_66", "dense_64", "edge", "zero")]


def identity_anchors(p, cand):
    """(anchors[B][T], the barcodes of at most 64 pairs): slot t < min(C, 4) of the scan holds v1 of the fit's slot t."""
    T = min(cand.shape[1], 4)
    return np.ascontiguousarray(cand[:, :T, 0]), np.flatnonzero(np.diff(p.sp.cell_pair_off) <= 64)


@pytest.mark.parametrize("case", IDENTITY_CASES, ids=CE.share_fit_id)
def test_fit_at_zero_is_the_scan_on_short_barcodes(m, case):
    """A barcode of at most 64 pairs leaves at most one term in each of the fit's 64 sums, so their fold is the scan's serial sum: the
    fit's evaluation at 0 of (v1, v2) is the scan's row of v2 under the anchor v1, bit for bit (NaN for NaN)."""
    name, Cn, _, _, _, _, given = case
    p = m["P"][name]
    val = result(m, "share_fit", case)[0]
    cand = CE.share_candidates(p, Cn)
    an, short = identity_anchors(p, cand)
    out = m["emu"].share_scan(p.sp, p.g, *tables(m, p), an, *soup(p, given))[0]
    n = 0
    for b in short:
        for t in range(an.shape[1]):
            if an[b, t] >= 0:
                assert same_bits_or_nan(val[b, t, 4:7], out[b, t, cand[b, t, 1]]), (b, t, val[b, t, 4:7], out[b, t, cand[b, t, 1]])
                n += 1
    assert n >= 3 and len(short) < p.sp.n_cells or name in ("edge", "zero", "dense_64")


def test_stage_vector_is_the_refinements(m):
    """One barcode per sample: the refinement's LL[i][v] is the stage's lgl of (i, that barcode), bit for bit."""
    p = m["P"]["mix_edges"]
    B, S = p.sp.n_cells, p.sp.n_snps
    ll = m["emu"].refine(p.sp, S, B, *tables(m, p), np.arange(B))[0]
    off, cell, lgl = m["emu"].cluster_stage(p.sp, *tables(m, p))[:3]
    snp = np.repeat(np.arange(S), np.diff(off))
    assert np.array_equal(CE.bits(ll[snp, cell]), CE.bits(lgl))


# ---- against 50-digit arithmetic -----------------------------------------------------------------------------------------------------------

def mp_problem(m):
    """test_mpmath_kat's second problem: 50 barcodes x 120 SNPs x 4 samples, GP field (the engine's converter)."""
    engine, synth = m["engine"], m["synth"]
    rng = np.random.default_rng(4242)
    B, S, V = 50, 120, 4
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([engine.geno_from_gp(x, 0.01) for x in synth.raw_gp_from_alleles(rng, raw.alleles)])
    sp = synth.make_pileup(rng, raw.alleles, B, 0.5, 1.8, dense_layout=False, doublet_rate=0.3)
    return CE.Problem("kat50", sp, g)


class Exact:
    """include/dmx.h's formulas in real-number arithmetic (mpmath, 50 digits): no binary64 rounding anywhere, no summation order."""

    def __init__(self, p, mat, err):
        mpmath.mp.dps = 50
        self.f = mpmath.mpf
        f = self.f
        sp = p.sp
        self.B, self.S, self.V = sp.n_cells, p.g.shape[0], p.g.shape[1]
        self.G = [[[f(float(p.g[s, v, k])) for k in range(3)] for v in range(self.V)] for s in range(self.S)]
        self.mat = [f(float(x)) for x in mat[:128]]
        self.e3 = [f(float(x)) / 3 for x in err[:128]]
        cell, snp, nrd, start = ambient_ref.host_pairs(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd)
        rd = np.asarray(sp.reads)
        self.pairs = [[] for _ in range(self.B)]                # per barcode: (snp, [(allele, bq), ...]) in stored order
        for c, s, n, st in zip(cell, snp, nrd, start):
            self.pairs[c].append((int(s), [(int(b) >> 7, int(b) & 127) for b in rd[st:st + n]]))

    def product(self, reads, p):
        """prod over the reads of pR (1 - p) + pA p"""
        x = self.f(1)
        for al, bq in reads:
            pR, pA = (self.e3[bq], self.mat[bq]) if al else (self.mat[bq], self.e3[bq])
            x *= pR * (1 - p) + pA * p
        return x

    def ambient(self, assign, a, grid):
        f = self.f
        LL = np.zeros((self.B, len(grid)))
        for b in range(self.B):
            v = int(assign[b])
            for q, rho in enumerate(grid):
                acc = f(0)
                for s, reads in self.pairs[b] if v >= 0 else []:
                    if not reads or not any(self.G[s][v]):
                        continue
                    acc += mpmath.log(sum(self.G[s][v][k] * self.product(reads, (1 - f(rho)) * k / 2 + f(rho) * f(a[s])) for k in range(3)))
                LL[b, q] = float(acc)
        return LL

    def mix(self, l, k, alpha, rho, a):
        f = self.f
        return (1 - f(rho)) * (f("0.5") * l + (k - l) * f("0.5") * f(alpha)) + f(rho) * f(a)

    def ambient_doublet(self, cand, alphas, a, grid):
        LL = np.zeros((self.B, cand.shape[1], len(alphas), len(grid)))
        for b in range(self.B):
            for c, (v1, v2) in enumerate(cand[b]):
                if v1 < 0:
                    continue
                for n, al in enumerate(alphas):
                    for q, rho in enumerate(grid):
                        acc = self.f(0)
                        for s, reads in self.pairs[b]:
                            if not reads or not any(self.G[s][v1]) or not any(self.G[s][v2]):
                                continue
                            acc += mpmath.log(sum(self.G[s][v1][l] * self.G[s][v2][k] * self.product(reads, self.mix(l, k, al, rho, a[s]))
                                                  for l in range(3) for k in range(3)))
                        LL[b, c, n, q] = float(acc)
        return LL

    def fit(self, hyp, alpha, rho, a, M):
        f = self.f
        out = np.zeros((3, self.B))
        for b in range(self.B):
            v1, v2 = int(hyp[b, 0]), int(hyp[b, 1])
            if v1 < 0:
                continue
            obs = mean = var = f(0)
            for s, reads in self.pairs[b]:
                if not reads or not any(self.G[s][v1]) or (v2 >= 0 and not any(self.G[s][v2])):
                    continue
                if v2 < 0:
                    comp = [(self.G[s][v1][k], (1 - f(rho[b])) * k / 2 + f(rho[b]) * f(a[s])) for k in range(3)]
                else:
                    comp = [(self.G[s][v1][l] * self.G[s][v2][k], self.mix(l, k, alpha[b], rho[b], a[s])) for l in range(3) for k in range(3)]
                first = reads[:M]
                mm = len(first)
                x = sum(al << r for r, (al, _) in enumerate(first))
                L = [sum(w * self.product([((y >> r) & 1, first[r][1]) for r in range(mm)], pc) for w, pc in comp) for y in range(1 << mm)]
                S0 = sum(L)
                lg = [mpmath.log(v) for v in L]
                e = sum(Ly * l for Ly, l in zip(L, lg)) / S0
                obs += lg[x]; mean += e; var += sum(Ly * (l - e) ** 2 for Ly, l in zip(L, lg)) / S0
            out[:, b] = [float(obs), float(mean), float(var)]
        return out

    def share(self, b, v1, v2, alpha, rho, a):
        """(LL, LL', LL'', m1, m2, N, n_max) of the pair (v1, v2) on barcode b at the share alpha: the header's formulas and the
        magnitudes test_gpu_share's bounds are stated in (share_ref's m1 and m2)."""
        f = self.f
        LL = D1s = D2s = m1 = m2 = f(0)
        N = n_max = 0
        for s, reads in self.pairs[b]:
            if not reads or not any(self.G[s][v1]) or not any(self.G[s][v2]):
                continue
            L = L1 = L2 = A1 = A2 = f(0)
            for l in range(3):
                for k in range(3):
                    w = self.G[s][v1][l] * self.G[s][v2][k]
                    if w == 0:
                        continue
                    p, sl = self.mix(l, k, alpha, rho, a[s]), (1 - f(rho)) * f("0.5") * (k - l)
                    fl, S1, S1a, S2 = f(1), f(0), f(0), f(0)
                    for al, bq in reads:
                        pR, pA = (self.e3[bq], self.mat[bq]) if al else (self.mat[bq], self.e3[bq])
                        t = pR * (1 - p) + pA * p
                        u = (pA - pR) / t
                        fl *= t; S1 += u; S1a += abs(u); S2 += u * u
                    L += w * fl; L1 += w * fl * sl * S1; L2 += w * fl * ((sl * S1) ** 2 - sl * sl * S2)
                    A1 += w * fl * abs(sl) * S1a; A2 += w * fl * ((abs(sl) * S1a) ** 2 + sl * sl * S2)
            LL += mpmath.log(L); D1s += L1 / L; D2s += L2 / L - (L1 / L) ** 2
            m1 += A1 / L; m2 += A2 / L + (A1 / L) ** 2
            N += 1; n_max = max(n_max, len(reads))
        return LL, D1s, D2s, float(m1), float(m2), N, n_max

    def site(self, hyp, alpha, rho, a, M):
        """obs / mean / var / exc / vexc [5][S]"""
        f = self.f
        out = [[f(0)] * self.S for _ in range(5)]
        for b in range(self.B):
            v1, v2 = int(hyp[b, 0]), int(hyp[b, 1])
            if v1 < 0:
                continue
            for s, reads in self.pairs[b]:
                if not reads or not any(self.G[s][v1]) or (v2 >= 0 and not any(self.G[s][v2])):
                    continue
                if v2 < 0:
                    comp = [(self.G[s][v1][k], (1 - f(rho[b])) * k / 2 + f(rho[b]) * f(a[s])) for k in range(3)]
                else:
                    comp = [(self.G[s][v1][l] * self.G[s][v2][k], self.mix(l, k, alpha[b], rho[b], a[s])) for l in range(3) for k in range(3)]
                first = reads[:M]
                mm = len(first)
                x = sum(al << r for r, (al, _) in enumerate(first))
                L = [sum(w * self.product([((y >> r) & 1, first[r][1]) for r in range(mm)], pc) for w, pc in comp) for y in range(1 << mm)]
                S0 = sum(L)
                lg = [mpmath.log(v) for v in L]
                e = sum(Ly * l for Ly, l in zip(L, lg)) / S0
                ky = [bin(y).count("1") for y in range(1 << mm)]
                a1 = sum(Ly * k for Ly, k in zip(L, ky)) / S0
                terms = (lg[x], e, sum(Ly * (l - e) ** 2 for Ly, l in zip(L, lg)) / S0, ky[x] - a1, sum(Ly * k * k for Ly, k in zip(L, ky)) / S0 - a1 * a1)
                for j, t in enumerate(terms):
                    out[j][s] += t
        return np.array([[float(x) for x in row] for row in out])

    def gl(self, reads):
        f = self.f
        g = [f(1)] * 3
        for al, bq in reads:
            g = [g[0] * (self.e3[bq] if al else self.mat[bq]), g[1] * (f("0.5") - self.e3[bq]), g[2] * (self.mat[bq] if al else self.e3[bq])]
        t = sum(g); g = [x / t for x in g]                                   # the per-read renormalisations telescope
        g = [x + f("1e-6") for x in g]; t = sum(g)
        return [mpmath.log(x / t) for x in g]

    def refine(self, assign):
        LL = [[[self.f(0)] * 3 for _ in range(self.V)] for _ in range(self.S)]
        for b in range(self.B):
            v = int(assign[b])
            for s, reads in self.pairs[b] if v >= 0 else []:
                LL[s][v] = [x + y for x, y in zip(LL[s][v], self.gl(reads))]
        return np.array([[[float(x) for x in r] for r in row] for row in LL])

    def cluster(self, w):
        """(lgl per slot in the stage's order, LL[S][C][3], W[S][C])"""
        Cn = w.shape[1]
        slots = sorted((s, b, k) for b in range(self.B) for k, (s, _) in enumerate(self.pairs[b]))
        lg = [self.gl(self.pairs[b][k][1]) for s, b, k in slots]
        LL = [[[self.f(0)] * 3 for _ in range(Cn)] for _ in range(self.S)]
        W = [[self.f(0)] * Cn for _ in range(self.S)]
        for (s, b, _), l in zip(slots, lg):
            for c in range(Cn):
                x = self.f(float(w[b, c]))
                LL[s][c] = [acc + x * y for acc, y in zip(LL[s][c], l)]
                W[s][c] += x
        return (np.array([[float(x) for x in l] for l in lg]), np.array([[[float(x) for x in r] for r in row] for row in LL]),
                np.array([[float(x) for x in row] for row in W]))


def test_against_50_digit_arithmetic(m):
    p = mp_problem(m)
    mat, err = m["mat"], m["err"]
    emu, ex = m["emu"], Exact(p, mat, err)
    B, V = p.sp.n_cells, p.V
    rng = np.random.default_rng(77)
    a = CE.amb_freq(p)
    assign = CE.assignment(p)
    grid = np.array([0.0, 0.1, 0.5])
    d = {}
    ll, _, _, c1 = emu.ambient(p.sp, p.g, mat, err, assign, a, grid)
    d["ambient LL"] = np.abs(ll - ex.ambient(assign, a, grid)).max()
    cand = CE.candidates(p, 2)
    alphas, grid2 = np.array([0.37, 0.5]), np.array([0.0, 0.2])
    ll, _, _, c2 = emu.ambient_doublet(p.sp, p.g, mat, err, cand, alphas, a, grid2)
    d["ambient doublet LL"] = np.abs(ll - ex.ambient_doublet(cand, alphas, a, grid2)).max()
    hyp, alpha, rho = CE.hypotheses(p)
    out, c3 = emu.fit(p.sp, p.g, mat, err, hyp, alpha, rho, a, 4)
    want = ex.fit(hyp, alpha, rho, a, 4)
    assert out["n_zero"].sum() == 0
    for i, k in enumerate(("obs", "mean", "var")):
        d[f"fit {k}"] = np.abs(out[k] - want[i]).max()
    ll = emu.refine(p.sp, p.g.shape[0], V, mat, err, assign)[0]
    d["refine LL"] = np.abs(ll - ex.refine(assign)).max()
    w = CE.mstep_weights(p, 3)
    off, cell, lgl = emu.cluster_stage(p.sp, mat, err)[:3]
    LL, W = emu.cluster_mstep(off, cell, lgl, w)
    xlgl, xLL, xW = ex.cluster(w)
    d["cluster lgl"] = np.abs(lgl - xlgl).max()
    d["cluster M-step LL"] = np.abs(LL - xLL).max()
    d["cluster M-step W"] = np.abs(W - xW).max()
    # the share scan and fit: LL at 1e-12; LL' and LL'' grow like 1 / err and hold test_gpu_share's U k1 m1 and U k2 m2, with m1, m2, N and
    # n_max taken from the 50-digit run itself
    rho_b = CE.barcode_rho(p)
    rho_b[rho_b == 1.0] = 0.3                       # (at rho = 1 every derivative is exactly 0: nothing to measure)
    an = CE.anchors(p, 1)
    out, _, c4 = emu.share_scan(p.sp, p.g, mat, err, an, rho_b, a)
    val, cts, _, c5 = emu.share_fit(p.sp, p.g, mat, err, cand, rho_b, a, 0.5, 1e-6, 30, 0.37)
    U = TS.U
    share = {"scan": [0.0, 0.0, 0.0], "fit": [0.0, 0.0, 0.0]}

    def against(what, got, b, v1, v2, al):
        LL, D1, D2, m1, m2, N, n = ex.share(b, v1, v2, al, rho_b[b], a)
        bound = (TOL_MP, U * (9 * n + 20 + N + 63) * m1, U * (2 * (9 * n + 20) + 2 + N + 63) * m2)
        for j, x in enumerate((LL, D1, D2)):
            dj = abs(float(mpmath.mpf(float(got[j])) - x))
            d[f"share {what} {('LL', 'LL_1', 'LL_2')[j]}"] = max(d.get(f"share {what} {('LL', 'LL_1', 'LL_2')[j]}", 0.0), dj)
            if bound[j] > 0:
                share[what][j] = max(share[what][j], dj / bound[j])
            assert dj <= bound[j], (what, b, v1, v2, al, j, dj, bound[j])

    for b in range(0, B, 3):
        if an[b, 0] >= 0:
            for v in range(V):
                if v != an[b, 0]:
                    against("scan", out[b, 0, v], b, int(an[b, 0]), v, 0.0)
        for c in range(2):
            if cand[b, c, 0] >= 0:
                for o, al in ((1, float(val[b, c, 0])), (4, 0.0), (7, 1.0), (10, 0.37)):
                    against("fit", val[b, c, o:o + 3], b, int(cand[b, c, 0]), int(cand[b, c, 1]), al)
    assert (cts[:, :, 1] & CE.INTERIOR).any()
    print(f"largest share of U k1 m1 / U k2 m2: scan LL' {share['scan'][1]:.3f}, LL'' {share['scan'][2]:.3f}; fit LL' {share['fit'][1]:.3f}, "
          f"LL'' {share['fit'][2]:.3f}")
    derivative = {k: d.pop(k) for k in list(d) if k.endswith(("LL_1", "LL_2"))}      # (held to their own bounds above, not to 1e-12)
    for k, v in derivative.items():
        print(f"emulator vs 50-digit arithmetic, {k}: max |delta| = {v:.2e}")
    # the site audit: the five sums per SNP at 1e-12
    sout, c6 = emu.site_fit(p.sp, p.g, mat, err, hyp, alpha, rho, a, 4)
    want = ex.site(hyp, alpha, rho, a, 4)
    assert sout["n_zero"].sum() == 0 and sout["n_cell"].sum() > 1000
    for i, k in enumerate(CE.SITE_FLOATS):
        d[f"site {k}"] = np.abs(sout[k] - want[i]).max()
    for c in (c1, c2, c3, c4, c5, c6):
        assert c["log_zero"] == 0 and c["log_other"] == 0
    for k, v in d.items():
        print(f"emulator vs 50-digit arithmetic, {k}: max |delta| = {v:.2e}")
    for k, v in d.items():
        assert v < TOL_MP, (k, v)


# ---- the inputs can tell -------------------------------------------------------------------------------------------------------------------

def differs(x, y):
    """some output's bits differ (the counters, the last element of a result, are not outputs)"""
    return any(not np.array_equal(CE.bits(a), CE.bits(b)) for a, b in zip(x[:-1], y[:-1]))


@pytest.mark.parametrize("pas", list(PASSES))
@pytest.mark.parametrize("wrong", ["contract", "descending", "libm_log"])
def test_inputs_tell_wrong_variants_apart(m, pas, wrong):
    which, variant = {"contract": ("fast", 0), "descending": ("emu", CE.DESCENDING), "libm_log": ("emu", CE.LIBM_LOG)}[wrong]
    hit = [case for case in PASSES[pas][1] if differs(result(m, pas, case), result(m, pas, case, which, variant))]
    print(f"{pas}, {wrong}: {len(hit)} of {len(PASSES[pas][1])} cases change bits")
    assert hit, f"no case of {pas} notices the variant '{wrong}'"


# ---- conditions on the inputs --------------------------------------------------------------------------------------------------------------

def test_log_arguments_and_rescales(m):
    for pas, (_, cases) in PASSES.items():
        for case in cases:
            cnt = result(m, pas, case)[-1]
            name = case if isinstance(case, str) else case[0]
            assert cnt["log_other"] == 0, (pas, case, cnt)
            profile = pas in ("ambient", "ambient_doublet", "share_scan", "share_fit")
            if name == "zero":
                if profile:
                    assert cnt["log_zero"] > 0 and np.isneginf(result(m, pas, case)[0]).any()
                if pas in ("share_scan", "share_fit"):                       # L = 0: lg = -inf and D1, D2 are NaN
                    assert np.isnan(result(m, pas, case)[0]).any()
            else:
                assert cnt["log_zero"] == 0, (pas, case, cnt)
            if profile and m["P"][name].deep:
                assert cnt["rescales"] > 0, (pas, case, cnt)
            if profile and name != "zero":
                assert np.isfinite(result(m, pas, case)[0]).all()


def test_fit_reaches_truncation_and_zero_likelihood(m):
    n_trunc = sum(int(result(m, "fit", case)[5].sum()) for case in CE.FIT_CASES)
    n_zero = {case: int(result(m, "fit", case)[6].sum()) for case in CE.FIT_CASES}
    assert n_trunc > 0 and n_zero[("zero", 2, False)] > 0
    assert all(v == 0 for case, v in n_zero.items() if case[0] != "zero")
    deep = m["P"]["mix_edges"].sp
    assert int(np.asarray(deep.pair_nrd).max()) >= 256 and result(m, "fit", ("mix_edges", 8, True))[5].sum() > 0    # a truncated 300-read pair


def test_inputs_reach_every_shape(m):
    P = m["P"]
    for name in ("mix_full", "mix_edges", "mix_max"):
        counts = np.diff(P[name].sp.cell_pair_off)
        assert set(CE.PAIR_COUNTS) <= set(counts.tolist()), name
        assert set(QM.DEPTHS.tolist()) <= set(np.asarray(P[name].sp.pair_nrd).tolist()), name
    assert {P[n].sp.pair_nrd.dtype.itemsize for n in P} == {1, 2, 4}
    assert any(P[n].sp.pair_snp is None for n in P) and any(P[n].sp.pair_snp is not None for n in P)
    for name in ("mix_full", "edge"):
        g = P[name].g
        assert (g == 0).all(axis=2).any() and ((g == 0).any(axis=2) & (g != 0).any(axis=2)).any()
        assert ((g > 0) & (g < np.finfo(np.float32).tiny)).any()
    for name in ("mix_full", "mix_edges", "mix_max", "edge"):                # unused barcodes, slots and hypotheses
        assert (CE.assignment(P[name]) < 0).any() and (CE.hypotheses(P[name])[0][:, 0] < 0).any() or name == "edge"
        assert (CE.candidates(P[name], 3)[:, :, 0] < 0).any() or name == "edge"
    assert (CE.assignment(P["edge"]) < 0).any() and (CE.candidates(P["edge"], 8)[:, :, 0] < 0).any()
    assert sorted({c[1] for c in CE.AMBIENT_DBL_CASES}) == list(range(1, 9))
    assert {c[2] for c in CE.AMBIENT_DBL_CASES} == {1, 3} and all(0.37 in CE.ALPHAS[k] for k in CE.ALPHAS)
    assert {c[1] for c in CE.AMBIENT_CASES} >= {1, 64, 65} and {P[c[0]].V for c in CE.AMBIENT_CASES} >= {1, 5}
    for Q in (2, 3, 65):
        assert CE.GRIDS[Q][0] == 0.0 and CE.GRIDS[Q][-1] == 1.0
    assert all((CE.amb_freq(P[n]) == 0).any() for n in P) and all((CE.amb_freq(P[n]) == 1).any() for n in P if P[n].g.shape[0] > 3)
    assert {c[1] for c in CE.MSTEP_CASES} == {1, 3, 70}
    assert {c[1] for c in CE.FIT_CASES} == {1, 2, 3, 4, 5, 8}
    assert {7, 8, 9, 40, 300} <= set(np.asarray(P["edge"].sp.pair_nrd).tolist())
    for S in (511, 512, 513):
        assert P[f"slab_{S}"].g.shape[0] == S
        assert {1, 2, 3, 14, 15, 16, 17, 40} <= set(np.asarray(P[f"slab_{S}"].sp.pair_nrd).tolist())


def test_share_inputs_reach_every_shape_and_branch(m):
    P = m["P"]
    # the scan: the panel's second block of partners, the ids around the block's edge, every T, unused slots, every nrd width, rho absent and given
    panel = P["panel_66"]
    assert panel.V == 66 and set(CE.PAIR_COUNTS) <= set(np.diff(panel.sp.cell_pair_off).tolist()) and int(np.asarray(panel.sp.pair_nrd).max()) >= 256
    assert {c[1] for c in CE.SHARE_SCAN_CASES if c[0] == "panel_66"} == {1, 2, 4} == {c[1] for c in CE.SHARE_SCAN_CASES}
    seen = set()
    for T in (1, 2, 4):
        an = CE.anchors(panel, T)
        assert (an < 0).any()
        seen |= set(an[an >= 0].tolist())
    assert {63, 64, 65} <= seen and any(v < 63 for v in seen)
    assert {P[c[0]].V for c in CE.SHARE_SCAN_CASES} >= {2, 3, 5, 66}
    assert {P[c[0]].sp.pair_nrd.dtype.itemsize for c in CE.SHARE_SCAN_CASES} == {1, 2, 4} == {P[c[0]].sp.pair_nrd.dtype.itemsize for c in CE.SHARE_FIT_CASES}
    assert {c[2] for c in CE.SHARE_SCAN_CASES} == {True, False} == {c[6] for c in CE.SHARE_FIT_CASES}
    assert set(CE.barcode_rho(panel).tolist()) == {0.0, 0.05, 0.3, 1.0}
    # the fit: every argument value, unused slots, the pool on both sides of 64 pairs with deep pairs
    assert {c[1] for c in CE.SHARE_FIT_CASES} == {1, 3, 8} and {c[2] for c in CE.SHARE_FIT_CASES} == {0.5, 0.2}
    assert {c[3] for c in CE.SHARE_FIT_CASES} == {1e-6, 1e-2} and {c[4] for c in CE.SHARE_FIT_CASES} == {1, 2, 30}
    assert {c[5] for c in CE.SHARE_FIT_CASES} == {-1.0, 0.0, 0.5, 1.0}
    pool = P["pool_02"]
    n_pair = np.diff(pool.sp.cell_pair_off)
    assert 24 <= pool.sp.n_cells <= 48 and (n_pair > 64).sum() >= 10 and (n_pair <= 64).sum() >= 4 and set(CE.POOL_COUNTS) <= set(n_pair.tolist())
    assert (np.asarray(pool.sp.pair_nrd) == 280).sum() >= 5 and (pool.sp.truth[:, 1] >= 0).all()
    for Cn in (3, 8):
        assert (CE.share_candidates(pool, Cn)[:, :, 0] < 0).any() and (CE.share_candidates(P["mix_full"], Cn)[:, :, 0] < 0).any()
    # every status bit, every way out of the driver, a refused Newton step, interior maxima after three or more evaluations of step 6
    status, how = set(), set()
    step2_ends, refused, long_interior = set(), 0, 0
    for case in CE.SHARE_FIT_CASES:
        name, Cn, start, tol, max_iter, probe, given = case
        p = P[name]
        cand = CE.share_candidates(p, Cn)
        val, cts, tr, _ = m["emu"].share_fit(p.sp, p.g, *tables(m, p), cand, *soup(p, given), start, tol, max_iter, probe)
        used = cand[:, :, 0] >= 0
        st, ne = cts[:, :, 1][used], cts[:, :, 0][used]
        for bit in (CE.INTERIOR, CE.AT_0, CE.AT_1, CE.NOT_CONVERGED, CE.FLAT, CE.NONFINITE):
            if (st & bit).any():
                status.add(bit)
        how |= set(tr[:, :, 0][used].tolist())
        step2 = tr[:, :, 0][used] == 2
        step2_ends |= set((st[step2] & (CE.AT_0 | CE.AT_1)).tolist())
        refused += int(tr[:, :, 2][used].sum())
        long_interior += int((((st & CE.INTERIOR) != 0) & ((st & CE.NOT_CONVERGED) == 0) & (ne >= 2 + 3 + 1)).sum())
        assert ((st & CE.NONFINITE) != 0).any() == (name == "zero")
        assert (ne[(st & CE.INTERIOR) == 0] == 2).all() and (ne[(st & CE.INTERIOR) != 0] >= 4).all()      # the probe is not counted
    print(f"share fit: {refused} bisection steps where a Newton step was refused, {long_interior} interior slots after >= 3 evaluations of step 6")
    assert status == {CE.INTERIOR, CE.AT_0, CE.AT_1, CE.NOT_CONVERGED, CE.FLAT, CE.NONFINITE}
    assert how == {1, 2, 3, 4, 10} and step2_ends == {CE.AT_0, CE.AT_1}
    assert refused >= 1 and long_interior >= 20


def test_site_inputs_reach_every_shape(m):
    P = m["P"]
    lens = {0: set(), 1: set()}
    kinds_at_M = {}
    chunks3 = nobody = False
    for case in CE.SITE_CASES:
        name, M, given, lists = case
        p = P[name]
        hyp, alpha, rho, a, _ = site_arguments(p, case)
        sng, dbl = site_ref.listing(hyp)
        if name.startswith("slab_"):
            lens[0].add(len(sng)); lens[1].add(len(dbl))
            assert (hyp[:, 0] < 0).any() and (hyp[hyp[:, 0] >= 0, 0] != np.flatnonzero(hyp[:, 0] >= 0) % p.V).any()     # unused, and wrong ones
        kinds_at_M.setdefault(M, set()).update(([0] if len(sng) else []) + ([1] if len(dbl) else []))
        n_cell = result(m, "site_fit", case)[5]
        nobody |= bool((n_cell == 0).any())
        if len(sng) > 128 or len(dbl) > 128:                                  # a SNP whose pairs come from three chunks of one list
            cell = np.repeat(np.arange(p.sp.n_cells), np.diff(p.sp.cell_pair_off))
            lst = sng if len(sng) > 128 else dbl
            pos = np.full(p.sp.n_cells, -1); pos[lst] = np.arange(len(lst)) // 64
            per_snp = {}
            for c, s_ in zip(cell, np.asarray(p.sp.pair_snp)):
                if pos[c] >= 0:
                    per_snp.setdefault(int(s_), set()).add(int(pos[c]))
            chunks3 |= any(len(v) >= 3 for v in per_snp.values())
        if name == "slab_513":
            assert n_cell[511] > 0 and n_cell[512] > 0
    assert lens[0] == set(CE.LIST_LENGTHS) == lens[1]
    assert set(kinds_at_M) == {1, 2, 3, 4, 5, 8} and all(v == {0, 1} for v in kinds_at_M.values()), kinds_at_M
    assert chunks3 and nobody
    assert {c[2] for c in CE.SITE_CASES} == {True, False} and ("dense_65", 4, True, None) in CE.SITE_CASES and ("edge", 8, True, None) in CE.SITE_CASES
    assert set(CE.site_hypotheses(P["slab_511"], (0, 129))[1].tolist()) == {0.0, 0.5, 0.37}
    assert result(m, "site_fit", ("zero", 2, False, None))[9].sum() > 0 and CE.SITE_WAVES_CASE in CE.SITE_CASES
    assert all(result(m, "site_fit", c)[9].sum() == 0 for c in CE.SITE_CASES if c[0] != "zero")
    # dense_65: six barcodes in one chunk at every SNP
    h65 = site_arguments(P["dense_65"], ("dense_65", 4, True, None))[0]
    assert P["dense_65"].sp.pair_snp is None and (h65[:, 0] >= 0).sum() >= 4
