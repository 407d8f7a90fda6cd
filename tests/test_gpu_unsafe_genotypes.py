"""GPU (-m gpu): genotype matrices that are not "safe" — a row with a NaN, an infinity, a negative entry or no entry >= 1e-30f.

dmx_engine_set_genotypes' k_check_geno finds such a row and the whole dispatch changes: every K2 family runs its checked (CHK) form,
whose barcodes that meet a log() argument outside the normal positive range are flagged and recomputed by k_doublet_generic<FIXUP>
with ocml's log(); K1 patches the term in place (log_slow); k_doublet_a2u / a2u16 / a2s and the lean k_singlet_can / k_singlet_canp
are never launched.  The results hold -inf, +inf and NaN, and K3, the finaliser and the .pair formatter see them.

Every kernel family of quality_mix.FAMILIES runs the problem of family_problem (quals = "edges") with a poisoned matrix
(unsafe_geno.poison: all-zero rows -> -inf; a NaN SNP, a negative, a +inf and a denormal entry -> NaN / +inf) against the oracle:
finite entries within 1e-9, non-finite ones of the same class at the same position.  The barcodes that cover no poisoned SNP must
keep the bits of the unpoisoned run under DMX_FORCE_CHECK=1 (the same dispatch with nothing flagged): a flag or a fix-up that leaks
across the barcodes of one workgroup shows there.  UNSAFE_NAMES records which kernels an unsafe matrix runs, per family."""
import numpy as np
import pytest

from golden_util import printed_mask
from quality_mix import A2, A3, FAMILIES, family_problem, genotypes, host_pileup, mixed_depth_pileup, oracle_csr, oracle_run
from unsafe_geno import assert_matches, covered_snps, covering, is_safe, poison

pytestmark = pytest.mark.gpu
TOL = 1e-9
SWITCHES = ("DMX_K1_CANP", "DMX_A2_NO_SYMU", "DMX_A2_SYM", "DMX_NO_ANF", "DMX_K2_GENERIC", "DMX_FORCE_CHECK", "DMX_PAIR_ON_HOST", "DMX_RANGE_BYTES")
NEVER = ("k_doublet_a2u<", "k_doublet_a2u16", "k_doublet_a2s<", "k_singlet_can<", "k_singlet_canp<")
CLASS_KERNELS = ("k_singlet_cls", "k_doublet_cls")        # (prefixes: k_singlet_cls / clsw, k_doublet_cls / clsp / clsym / clsn)

# case id -> (K1, K2) an UNSAFE matrix runs (launch_singlet / launch_doublet with geno_safe false).  The lean canonical K1 kernels and the
# unordered-pair K2 kernels need a safe matrix: their families fall to k_singlet_cls<.., CAN = false> and k_doublet_a2<.., CHK = true>.
UNSAFE_NAMES = {
    "k1_singlet": ("k_singlet<1, 8, false>", "k_doublet_a2<64, 1, 1, false, true, 32>"),
    "k1_singlet_own": ("k_singlet_own<16, false, true>", "k_doublet_a2<64, 4, 1, false, true, 32>"),
    "k1_singlet_cls": ("k_singlet_cls<1, 8, false>", "k_doublet_cls<256, 4, 1, false>"),
    "k1_singlet_can": ("k_singlet_cls<1, 8, false>", "k_doublet_cls<64, 1, 1, false>"),
    "k1_singlet_canp": ("k_singlet_cls<1, 8, false>", "k_doublet_cls<64, 1, 1, false>"),
    "k1_singlet_clsw": ("k_singlet_clsw<1, 4, false>", "k_doublet_clsp<3, false>"),
    "k1_wide_v129_gp": ("k_singlet<1, 8, false>", "k_doublet_a2<256, 16, 1, false, true, 32>"),
    "k1_wide_v129_gt": ("k_singlet_clsw<1, 4, false>", "k_doublet_cls<256, 16, 1, false>"),
    "k2_cls_v24": ("k_singlet_clsw<1, 4, false>", "k_doublet_cls<256, 4, 1, false>"),
    "k2_clsp_fast": ("k_singlet_clsw<1, 4, false>", "k_doublet_clsp<3, true>"),
    "k2_clsym": ("k_singlet_cls<1, 8, false>", "k_doublet_clsym<1, 4>"),
    "k2_clsym_v24": ("k_singlet_clsw<1, 4, false>", "k_doublet_clsym<7, 3>"),
    "k2_clsn": ("k_singlet_cls<1, 8, false>", "k_doublet_clsn<256, 1, 4>"),
    "k2_a2u16": ("k_singlet_own<16, false, true>", "k_doublet_a2<64, 4, 1, false, true, 32>"),
    "k2_a2u": ("k_singlet_own<32, false, true>", "k_doublet_a2<256, 4, 4, true, true, 32>"),
    "k2_a2": ("k_singlet_own<32, true, true>", "k_doublet_a2<256, 4, 4, true, true, 32>"),
    "k2_a2s": ("k_singlet_own<32, false, true>", "k_doublet_a2<256, 4, 4, true, true, 32>"),
    "k2_sym_v8": ("k_singlet<1, 8, false>", "k_doublet_sym<16, 8, 4, true, 3, 0, true>"),
    "k2_sym_v32": ("k_singlet_own<32, true, true>", "k_doublet_sym<64, 32, 4, true, 3, 0, true>"),
    "k2_an": ("k_singlet_own<16, false, true>", "k_doublet_an<64, 4, 4>"),
    "k2_anf": ("k_singlet_own<16, false, true>", "k_doublet_anf<256, 1, 4, 16, 8, 3, true>"),
    "k2_a2f": ("k_singlet_own<16, false, true>", "k_doublet_a2f<64, 4>"),
    "k2_generic": ("k_singlet<1, 8, false>", "k_doublet_generic<unsigned short, 1, false>"),
    # the dense families of the two-barcode kernel and k_doublet_a2u16: the A2U switches select nothing without a safe matrix
    "k2_a2u2": ("k_singlet_own<32, true, true>", "k_doublet_a2<256, 4, 4, true, true, 32>"),
    "k2_a2u2_diag_behind": ("k_singlet_own<32, true, true>", "k_doublet_a2<256, 4, 4, true, true, 32>"),
    "k2_a2u2_mirror_fallback": ("k_singlet_own<32, true, true>", "k_doublet_a2<256, 4, 4, true, true, 32>"),
    "k2_a2u_dense_one_barcode": ("k_singlet_own<32, true, true>", "k_doublet_a2<256, 4, 4, true, true, 32>"),
    "k2_a2u16_dense": ("k_singlet_own<16, true, true>", "k_doublet_a2<64, 4, 1, false, true, 32>"),
    "k2_a2u16_mirror_fallback": ("k_singlet_own<16, true, true>", "k_doublet_a2<64, 4, 1, false, true, 32>"),
}
BY_CASE = {f[0]: f for f in FAMILIES}
ARRAYS = ("llks", "llk0s", "grid", "l00")


@pytest.fixture(scope="module")
def eng():
    from demuxlet_amd import build, capi, engine
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return engine


def run_engine(eng, monkeypatch, g, sp, alphas, mode, env):
    from demuxlet_amd import capi
    monkeypatch.setenv("DMX_EXPERIMENTS", "1")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = eng.Engine(g.shape[1], alphas, 0.5, mode=capi.DMX_MODE_FAST if mode == "fast" else capi.DMX_MODE_STRICT)
    e.set_genotypes(g); e.set_pileup(host_pileup(eng, sp)); e.run(); e.sync()
    names = e.kernel_names()
    llks, llk0s = e.get_singlet()
    grid, l00, summ = e.get_doublet()
    e.close()
    return dict(llks=llks, llk0s=llk0s, grid=grid, l00=l00, summ=summ, names=names)


def compare(out, ref, alphas, mode, what, rows=None):
    """assert_matches over the four arrays (FAST: the printed grid entries); returns (finite, non-finite, largest finite |d|)."""
    V, A = out["grid"].shape[1], len(alphas)
    proc = ref.processed.astype(bool)
    if rows is not None:
        proc = proc & rows
    gm = (printed_mask(V, A)[None] if mode == "fast" else np.ones((1, V, V, A), dtype=bool)) & proc[:, None, None, None]
    tot = [0, 0, 0.0]
    for name, r, m in (("llks", ref.llks, proc[:, None]), ("llk0s", ref.llk0s, proc), ("grid", ref.llksAB, gm), ("l00", ref.llks00, proc[:, None])):
        nf, nn, w = assert_matches(out[name], r, np.broadcast_to(m, r.shape), TOL, f"{what} {name}")
        tot = [tot[0] + nf, tot[1] + nn, max(tot[2], w)]
    return tuple(tot)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


_clean_runs = {}


def clean_run(eng, monkeypatch, case):
    """The unpoisoned problem of a family under DMX_FORCE_CHECK=1 (the dispatch of an unsafe matrix, nothing flagged) — once per family."""
    if case not in _clean_runs:
        _, field, V, alphas, mode, env, _, _, dense, deep = BY_CASE[case]
        g, sp = family_problem(eng, case, field, V, dense, deep, "edges")
        _clean_runs[case] = run_engine(eng, monkeypatch, g, sp, alphas, mode, {**env, "DMX_FORCE_CHECK": "1"})
    return _clean_runs[case]


@pytest.mark.parametrize("kind", ["zero", "nan"])
@pytest.mark.parametrize("case,field,V,alphas,mode,env,k1,k2,dense,deep", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_unsafe_matrix_every_family_against_oracle(eng, oracle, monkeypatch, case, field, V, alphas, mode, env, k1, k2, dense, deep, kind):
    """(a) a poisoned matrix through every family: values and non-finite classes as the oracle's, the checked kernels by name;
    (b) sparse pileups: the barcodes without a poisoned SNP keep the bits of the unpoisoned DMX_FORCE_CHECK=1 run."""
    g, sp = family_problem(eng, case, field, V, dense, deep, "edges")
    gp, snps = poison(g, kind, np.random.default_rng(sum(map(ord, case + kind))), sp)
    assert not is_safe(gp) and is_safe(g)
    ref = oracle_run(oracle, sp, gp, alphas)
    proc = ref.processed.astype(bool)
    cov = covering(sp, snps)
    # the case cannot pass vacuously
    assert (~np.isfinite(ref.llksAB[proc])).any() and (~np.isfinite(ref.llks[proc])).any()
    if kind == "zero":
        assert not np.isnan(ref.llksAB).any() and not np.isnan(ref.llks).any() and not np.isposinf(ref.llksAB).any()
    else:
        all_nan = np.isnan(ref.llks).all(axis=1) & np.isnan(ref.llksAB).all(axis=(1, 2, 3)) & np.isnan(ref.llk0s) & np.isnan(ref.llks00).all(axis=1)
        assert np.array_equal(all_nan, covering(sp, [snps[1]]))
    clean = proc & ~cov
    if not dense:
        assert clean.sum() >= 2
    if field == "GT":           # one bad row per SNP: still <= 4 bitwise-distinct rows, the class kernels stay selected
        assert max(len({r.tobytes() for r in gp[s]}) for s in range(gp.shape[0])) <= 4

    out = run_engine(eng, monkeypatch, gp, sp, alphas, mode, env)
    names = out["names"]
    nf, nn, worst = compare(out, ref, alphas, mode, f"{case} {kind}")
    _, _, worst_flagged = compare(out, ref, alphas, mode, f"{case} {kind} poisoned barcodes", rows=cov)
    print(f"{case} {kind}: {names['singlet']} | {names['doublet']} | {names['certify']}: finite {nf} non-finite {nn} "
          f"max|d| {worst:.2e} (barcodes with a poisoned SNP {worst_flagged:.2e}), {int(clean.sum())} clean barcodes")
    assert (names["singlet"], names["doublet"]) == UNSAFE_NAMES[case], names
    assert not any(names[k].startswith(p) for k in ("singlet", "doublet") for p in NEVER), names
    if field == "GT":
        assert names["singlet"].startswith(CLASS_KERNELS[0]) and names["doublet"].startswith(CLASS_KERNELS[1]), names

    if not dense:
        base = clean_run(eng, monkeypatch, case)
        assert (base["names"]["singlet"], base["names"]["doublet"]) == UNSAFE_NAMES[case], base["names"]
        for a in ARRAYS:
            assert same_bits(out[a][clean], base[a][clean]), (case, kind, a, np.flatnonzero(clean))


EDGE_FAMILIES = ["k1_singlet_can", "k2_a2u", "k2_cls_v24", "k2_sym_v8"]


@pytest.mark.parametrize("case", EDGE_FAMILIES)
def test_rows_at_the_edge_of_the_safe_range(eng, oracle, monkeypatch, case):
    """(c) a row whose maximum is exactly float32(1e-30) keeps the matrix safe (the unchecked kernels by name: k_doublet_a2u at 32 GP
    samples, the lean k_singlet_can, k_doublet_sym<.., CHK = false>); one float32 below, the matrix is unsafe and runs the checked set.
    Either way every result is finite and within 1e-9.  A GT matrix with gt_error = 0 (one-hot rows, hard zeros) is safe as well."""
    _, field, V, alphas, mode, env, k1, k2, dense, deep = BY_CASE[case]
    g, sp = family_problem(eng, case, field, V, dense, deep, "edges")
    rng = np.random.default_rng(sum(map(ord, case)))
    variants = [("at 1e-30f", poison(g, "edge_safe", rng, sp)[0], True), ("below 1e-30f", poison(g, "edge_safe", rng, sp, below=True)[0], False)]
    if field == "GT":
        raw_rng = np.random.default_rng(31000 + 7 * V + sum(map(ord, case)) + 1)     # family_problem's own draw of the alleles
        from demuxlet_amd import synth
        alleles = synth.make_raw_genotypes(raw_rng, g.shape[0], V).alleles
        g0 = genotypes(eng, raw_rng, alleles, "GT", gt_error=0.0)
        assert set(np.unique(g0)) == {0.0, 1.0} and np.array_equal(g0.argmax(axis=2), g.argmax(axis=2))
        variants.append(("one-hot", g0, True))
    for tag, gm, safe in variants:
        assert is_safe(gm) == safe, tag
        ref = oracle_run(oracle, sp, gm, alphas)
        for a in (ref.llks, ref.llk0s, ref.llksAB, ref.llks00):
            assert np.isfinite(a).all(), tag
        out = run_engine(eng, monkeypatch, gm, sp, alphas, mode, env)
        names = out["names"]
        nf, nn, worst = compare(out, ref, alphas, mode, f"{case} {tag}")
        print(f"{case} {tag}: {names['singlet']} | {names['doublet']}: finite {nf} max|d| {worst:.2e}")
        assert nn == 0
        if safe:
            assert names["singlet"].startswith(k1) and names["doublet"].startswith(k2), (tag, names)
            if k2 == "k_doublet_sym<":
                assert names["doublet"].endswith(", false>"), (tag, names)
        else:
            assert (names["singlet"], names["doublet"]) == UNSAFE_NAMES[case], (tag, names)


def small_problem(eng, seed, field, V, dup=None, S=300, B=24):
    from demuxlet_amd import synth
    rng = np.random.default_rng(seed)
    raw = synth.make_raw_genotypes(rng, S, V)
    if dup:
        raw.alleles[:, dup[1]] = raw.alleles[:, dup[0]]
    g = genotypes(eng, rng, raw.alleles, field)
    if dup:
        g[:, dup[1]] = g[:, dup[0]]
    return g, mixed_depth_pileup(rng, raw.alleles, B, 0.3)


def scans_defined(grid):
    """The reference's scans name a first and a second singlet and a best doublet: no NaN, two finite llksAB[j][0][0], one finite
    off-diagonal entry with n >= 1 (otherwise it indexes with -1)."""
    V = grid.shape[0]
    off = ~np.eye(V, dtype=bool)
    return bool(not np.isnan(grid).any() and np.isfinite(grid[:, 0, 0]).sum() >= 2 and np.isfinite(grid[off][:, 1:]).any())


@pytest.mark.parametrize("kind", ["zero", "nan"])
@pytest.mark.parametrize("V,alphas,field", [(5, A2, "GP"), (12, A3, "GT")])
def test_k3_records_of_grids_with_infinities_and_nans(eng, oracle, monkeypatch, V, alphas, field, kind):
    """(d) k_reduce over grids that hold -inf / +inf / NaN: where the reference's scans are defined the record equals their host
    restatement (test_gpu_parity.summary_from_grid) on the engine's own grid; an all-NaN barcode keeps its indices at -1 and the
    dependent values NaN."""
    from test_gpu_parity import summary_from_grid
    g, sp = small_problem(eng, 5200 + V, field, V)
    gp, snps = poison(g, kind, np.random.default_rng(V), sp)
    out = run_engine(eng, monkeypatch, gp, sp, alphas, "strict", {})
    ref = oracle_run(oracle, sp, gp, alphas)
    compare(out, ref, alphas, "strict", f"K3 V={V} {kind}")
    n_def = n_nonfinite = n_nan = 0
    for c in range(sp.n_cells):
        s, G = out["summ"][c], out["grid"][c]
        assert s["n_pairs"] == sp.cell_pair_off[c + 1] - sp.cell_pair_off[c]
        if np.isnan(G).all():
            n_nan += 1
            assert (s["i_sing1"], s["i_sing2"], s["j_best"], s["k_best"], s["n_best"]) == (-1, -1, -1, -1, -1)
            assert all(np.isnan(s[k]) for k in ("sing_llk1", "llk12", "llk1", "llk2", "llk10", "llk20", "llk00_0", "sum_single", "sum_double"))
            continue
        if not scans_defined(G):
            continue
        n_def += 1
        n_nonfinite += bool((~np.isfinite(G)).any())
        with np.errstate(invalid="ignore", over="ignore"):
            mx, ss, sd, i1, i2, (j, k, n) = summary_from_grid(G, out["l00"][c], alphas, 0.5)
        assert s["max_llk"] == mx
        assert (s["i_sing1"], s["i_sing2"], s["j_best"], s["k_best"], s["n_best"]) == (i1, i2, j, k, n)
        assert s["llk12"] == G[j, k, n] and s["llk10"] == G[j, 0, n] and s["llk20"] == G[k, 0, n]
        assert s["sing_llk1"] == G[i1, 0, 0] and s["sing_llk2"] == G[i2, 0, 0]
        for got, want in ((s["sum_single"], ss), (s["sum_double"], sd)):
            assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-12 * max(want, 1e-300), (c, got, want)
    print(f"K3 V={V} A={len(alphas)} {kind}: {n_def} barcodes with defined scans ({n_nonfinite} of them with non-finite entries), {n_nan} all-NaN")
    assert n_def >= 5 and n_nonfinite >= 2
    if kind == "nan":
        assert n_nan == covering(sp, [snps[1]]).sum() >= 1


def subset_pileup(sp, keep):
    """The pileup of the barcodes `keep` (ascending ids), same layout."""
    from demuxlet_amd import synth
    keep = np.asarray(keep)
    pi = np.concatenate([np.arange(sp.cell_pair_off[c], sp.cell_pair_off[c + 1]) for c in keep]).astype(np.int64)
    ri = np.concatenate([np.arange(sp.cell_read_off[c], sp.cell_read_off[c + 1]) for c in keep]).astype(np.int64)
    po = np.concatenate([[0], np.cumsum(np.diff(sp.cell_pair_off)[keep])]).astype(np.int64)
    ro = np.concatenate([[0], np.cumsum(np.diff(sp.cell_read_off)[keep])]).astype(np.int64)
    return synth.SynthPileup(len(keep), sp.n_snps, po, ro, sp.pair_snp[pi], sp.pair_nrd[pi], sp.reads[ri], sp.rd_totl[keep], sp.rd_pass[keep],
                             sp.rd_uniq[keep], sp.truth[keep])


def oracle_files(oracle, sp, g, alphas, bcs, sms, prefix):
    oracle.run_csr(oracle_csr(oracle, sp, bcs), sms, g, oracle.Params(tuple(alphas), 0.5, 0, 0, 0, True), str(prefix))
    return {suf: open(f"{prefix}.{suf}", "rb").read() for suf in ("single", "sing2", "best", "pair")}


def run_job(eng, monkeypatch, tmp_path, tag, sp, g, alphas, bcs, sms, mode, env):
    from demuxlet_amd import capi
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = eng.demuxlet_run(host_pileup(eng, sp), g, sms, alphas, str(tmp_path / tag), write_pair=True, barcodes=bcs,
                         mode=capi.DMX_MODE_FAST if mode == "fast" else capi.DMX_MODE_STRICT, timing=True)
    return {suf: (tmp_path / f"{tag}.{suf}").read_bytes() for suf in ("single", "sing2", "best", "pair")}, t


FILE_CASES = [(6, "GT"), (16, "GP")]


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("V,field", FILE_CASES)
def test_files_of_a_matrix_with_zero_rows(eng, oracle, monkeypatch, tmp_path, V, field, mode):
    """(e) dmx_demuxlet_run with --write-pair on all-zero rows (not sample 0's: the reference pairs every singlet entry with sample 0),
    one sample column duplicated so that near-tie flags meet -inf entries: the oracle's four files byte for byte, in one range and in
    many, and the same .pair bytes from the host formatter (DMX_PAIR_ON_HOST=1) as from the device's."""
    g, sp = small_problem(eng, 7000 + V, field, V, dup=(1, 2))
    gp, snps = poison(g, "zero", np.random.default_rng(1), sp, no_sample0=True)
    bcs = [f"BC{(i * 7919) % 100003:06d}-1" for i in range(sp.n_cells)]
    sms = [f"S{j:02d}" for j in range(V)]
    raw = oracle_run(oracle, sp, gp, A2)
    assert all(scans_defined(raw.llksAB[c]) for c in range(sp.n_cells))
    want = oracle_files(oracle, sp, gp, A2, bcs, sms, tmp_path / "orc")
    assert len({ln.split(b"\t")[0] for ln in want["pair"].splitlines() if b"-inf" in ln}) >= 5
    one, t1 = run_job(eng, monkeypatch, tmp_path, "one", sp, gp, A2, bcs, sms, mode, {})
    many, tm = run_job(eng, monkeypatch, tmp_path, "many", sp, gp, A2, bcs, sms, mode, {"DMX_RANGE_BYTES": "30000" if V == 16 else "4000"})
    host, _ = run_job(eng, monkeypatch, tmp_path, "host", sp, gp, A2, bcs, sms, mode, {"DMX_PAIR_ON_HOST": "1"})
    assert t1["n_ranges"] == 1 and tm["n_ranges"] > 2
    print(f"files V={V} {field} {mode}: {tm['n_ranges']} ranges, {t1['n_cells_grid_fetched']} grids fetched")
    for suf in ("single", "sing2", "best", "pair"):
        assert one[suf] == want[suf], suf
        assert many[suf] == one[suf] and host[suf] == one[suf], suf


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("V,field", FILE_CASES)
def test_files_of_a_matrix_with_a_nan_snp(eng, oracle, monkeypatch, tmp_path, V, field, mode):
    """(e) the missing-GP case end to end: the job succeeds, and every line of a barcode that does not cover the NaN SNP equals the
    oracle's for the pileup without the NaN barcodes (the reference's files are undefined for those: its scans index with -1)."""
    g, sp = small_problem(eng, 7000 + V, field, V, dup=(1, 2))
    gp, snps = poison(g, "nan", np.random.default_rng(1), sp, no_sample0=True)
    nan_bc = covering(sp, [snps[1]])
    keep = np.flatnonzero(~nan_bc)
    assert 2 <= len(keep) < sp.n_cells
    bcs = [f"BC{(i * 7919) % 100003:06d}-1" for i in range(sp.n_cells)]
    sms = [f"S{j:02d}" for j in range(V)]
    want = oracle_files(oracle, subset_pileup(sp, keep), gp, A2, [bcs[c] for c in keep], sms, tmp_path / "orc")
    kept = {bcs[c].encode() for c in keep}
    dev, _ = run_job(eng, monkeypatch, tmp_path, "dev", sp, gp, A2, bcs, sms, mode, {})
    host, _ = run_job(eng, monkeypatch, tmp_path, "host", sp, gp, A2, bcs, sms, mode, {"DMX_PAIR_ON_HOST": "1"})
    for suf in ("single", "sing2", "best", "pair"):
        lines = dev[suf].splitlines(keepends=True)
        assert b"".join([lines[0]] + [ln for ln in lines[1:] if ln.split(b"\t")[0] in kept]) == want[suf], suf
        assert len({ln.split(b"\t")[0] for ln in lines[1:]}) == sp.n_cells, suf
    assert host["pair"] == dev["pair"]


@pytest.mark.parametrize("V,field", FILE_CASES)
def test_records_path_with_zero_rows(eng, oracle, monkeypatch, tmp_path, V, field):
    """(e) the records route (K3 summaries + the near-tie barcodes' grids -> dmx_write_doublet_summary) on the zero-row problem:
    the oracle's .single / .sing2 / .best byte for byte."""
    g, sp = small_problem(eng, 7000 + V, field, V, dup=(1, 2))
    gp, _ = poison(g, "zero", np.random.default_rng(1), sp, no_sample0=True)
    bcs = [f"BC{(i * 7919) % 100003:06d}-1" for i in range(sp.n_cells)]
    sms = [f"S{j:02d}" for j in range(V)]
    want = oracle_files(oracle, sp, gp, A2, bcs, sms, tmp_path / "orc")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    pl = host_pileup(eng, sp)
    e = eng.Engine(V, A2, 0.5)
    e.set_genotypes(gp); e.set_pileup(pl); e.run(); e.sync()
    llks, llk0s = e.get_singlet()
    _, l00, summ = e.get_doublet(want_grid=False)
    sing = e.get_sing()
    near = eng.near_tie_cells(summ)
    grids = dict(zip(near.tolist(), e.get_cell_grids(near))) if len(near) else None
    e.close()
    fa = eng.FinalArgs(bcs, sms, A2, 0.5, sp.rd_totl, sp.rd_pass, sp.rd_uniq, np.diff(sp.cell_pair_off).astype(np.int32), 0, 0, 0, False)
    eng.write_single(fa, llks, llk0s, str(tmp_path / "o.single"))
    eng.write_doublet_summary(fa, sing, l00, summ, str(tmp_path / "o"), tie_pileup=pl, tie_g=gp, cell_grids=grids)
    print(f"records V={V} {field}: {len(near)} near-tie barcodes")
    for suf in ("single", "sing2", "best"):
        assert (tmp_path / f"o.{suf}").read_bytes() == want[suf], suf
