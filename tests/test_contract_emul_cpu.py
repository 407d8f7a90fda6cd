"""CPU: the host emulator of the feature passes' contracts (tests/contract_emul.cpp) is right before any kernel is judged by it.

On the inputs of tests/test_gpu_contract_bits.py (tests/contract_emul.py) the emulator is compared with the float64 numpy restatements
the tolerance tests use (ambient_ref, ambient_dbl_ref, fit_ref, ref_refine / pair_gl of test_gpu_refine, ref_stage / ref_mstep of
test_gpu_cluster) within those tests' own tolerances, counts exactly; on one problem of test_mpmath_kat's size (50 barcodes x 120 SNPs x
4 samples) with 50-digit arithmetic written from include/dmx.h's formulas, at that file's 1e-12.  Three deliberately wrong variants of the
emulator (products contracted into FMAs, descending order, libm's log) must each change bits of every pass on these inputs, and the
emulator's counters state the conditions the GPU comparison rests on: no subnormal / inf / nan log argument anywhere, zero arguments only
in the case built for them, rescales taken in the deep cases of both ambient passes, n_trunc and n_zero reached by the goodness of fit,
every depth regime of quality_mix.DEPTHS present.  No GPU compute is called.

Measured against 50-digit arithmetic (max |delta|, printed by test_against_50_digit_arithmetic): ambient LL 4.3e-14,
ambient doublet LL 4.3e-14, fit obs 1.1e-13 / mean 2.1e-14 / var 1.8e-13, refinement LL 2.8e-14, cluster lgl 1.8e-15, M-step LL 2.1e-14 / W
2.7e-15: every pass holds 1e-12."""
import mpmath
import numpy as np
import pytest

import ambient_dbl_ref
import ambient_ref
import contract_emul as CE
import fit_ref
import quality_mix as QM
import test_gpu_cluster as TC
import test_gpu_refine as TR

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


CLUSTER_CASES = [(n, None) for n in CE.REFINE_CASES] + CE.MSTEP_CASES
PASSES = {"ambient": (run_ambient, CE.AMBIENT_CASES), "ambient_doublet": (run_ambient_dbl, CE.AMBIENT_DBL_CASES), "fit": (run_fit, CE.FIT_CASES),
          "refine": (run_refine, CE.REFINE_CASES), "cluster": (run_cluster, CLUSTER_CASES)}


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
    for c in (c1, c2, c3):
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
            if name == "zero":
                if pas in ("ambient", "ambient_doublet"):
                    assert cnt["log_zero"] > 0 and np.isneginf(result(m, pas, case)[0]).any()
            else:
                assert cnt["log_zero"] == 0, (pas, case, cnt)
            if pas in ("ambient", "ambient_doublet") and m["P"][name].deep:
                assert cnt["rescales"] > 0, (pas, case, cnt)
            if pas in ("ambient", "ambient_doublet") and name != "zero":
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
