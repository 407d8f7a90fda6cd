"""CPU: the unsafe-matrix helper (tests/unsafe_geno.py) does what the GPU tests rely on — its poisons give the non-finite results they
claim (on the oracle), assert_matches tells the non-finite classes apart — and the host finaliser prints an oracle grid with -inf
entries as the oracle does."""
import numpy as np
import pytest

from quality_mix import A2, genotypes, mixed_depth_pileup, oracle_csr, oracle_run
from unsafe_geno import F32_BELOW, F32_EDGE, assert_matches, covering, is_safe, poison


@pytest.fixture(scope="module")
def eng():
    from demuxlet_amd import build, capi, engine
    build.build()
    capi.load()
    return engine


def problem(eng, V, field, dup=None, seed=5, S=300, B=24):
    from demuxlet_amd import synth
    rng = np.random.default_rng(seed)
    raw = synth.make_raw_genotypes(rng, S, V)
    if dup:
        raw.alleles[:, dup[1]] = raw.alleles[:, dup[0]]
    g = genotypes(eng, rng, raw.alleles, field)
    if dup:
        g[:, dup[1]] = g[:, dup[0]]
    return g, mixed_depth_pileup(rng, raw.alleles, B, 0.3)


@pytest.mark.parametrize("V,field", [(8, "GP"), (12, "GT")])
def test_poisons_produce_what_they_claim(eng, oracle, V, field):
    g, sp = problem(eng, V, field)
    safe = oracle_run(oracle, sp, g, A2)
    arrays = lambda r: (r.llks, r.llk0s, r.llksAB, r.llks00)
    assert is_safe(g) and all(np.isfinite(a).all() for a in arrays(safe))

    gz, snps = poison(g, "zero", np.random.default_rng(1), sp)
    assert not is_safe(gz) and len(snps) == 4 and (gz[snps[0], 0] == 0).all() and (gz[snps[3], V - 1] == 0).all()
    assert sorted(np.flatnonzero((gz != g).any(axis=(1, 2))).tolist()) == sorted(snps)
    z = oracle_run(oracle, sp, gz, A2)
    assert not any(np.isnan(a).any() or np.isposinf(a).any() for a in arrays(z))
    assert np.isneginf(z.llks).any() and np.isneginf(z.llksAB).any() and np.isfinite(z.llk0s).all() and np.isfinite(z.llks00).all()
    clean = ~covering(sp, snps)
    assert clean.sum() >= 2 and all(a[clean].tobytes() == b[clean].tobytes() for a, b in zip(arrays(z), arrays(safe)))
    # a zeroed row of sample 0 makes llksAB[j][0][0] -inf for every j (the reference pairs the singlet column with sample 0)
    c0 = covering(sp, [snps[0]])
    assert np.isneginf(z.llksAB[c0][:, :, 0, 0]).all()

    gn, snps = poison(g, "nan", np.random.default_rng(1), sp)
    assert not is_safe(gn) and np.isnan(gn[snps[1]]).all() and np.isposinf(gn).sum() == 1 and (gn < 0).sum() == 1
    n = oracle_run(oracle, sp, gn, A2)
    all_nan = np.isnan(n.llks).all(axis=1) & np.isnan(n.llksAB).all(axis=(1, 2, 3)) & np.isnan(n.llk0s) & np.isnan(n.llks00).all(axis=1)
    assert np.array_equal(all_nan, covering(sp, [snps[1]])) and all_nan.any() and not all_nan.all()
    only_denormal = covering(sp, [snps[3]]) & ~covering(sp, snps[:3])
    assert all(np.isfinite(a[only_denormal]).all() for a in arrays(n))

    for below, top in ((False, F32_EDGE), (True, F32_BELOW)):
        ge, snps = poison(g, "edge_safe", np.random.default_rng(1), sp, below=below)
        assert is_safe(ge) == (not below) and ge[snps[0], 0].max() == top and top > 0
        assert all(np.isfinite(a).all() for a in arrays(oracle_run(oracle, sp, ge, A2)))
    if field == "GT":           # one bad row per SNP: the class kernels' <= 4 bitwise-distinct rows survive every poison
        for gm in (gz, gn):
            assert max(len({r.tobytes() for r in gm[s]}) for s in range(gm.shape[0])) <= 4


def test_assert_matches_tells_the_classes_apart():
    ref = np.array([1.0, -np.inf, np.inf, np.nan, 2.0])
    assert assert_matches(ref.copy(), ref, None, 1e-9) == (2, 3, 0.0)
    assert assert_matches(ref + np.array([5e-10, 0, 0, 0, 0]), ref, None, 1e-9)[2] == pytest.approx(5e-10)
    assert assert_matches(np.array([7.0, np.nan]), np.array([1.0, np.nan]), np.array([False, True]), 1e-9) == (0, 1, 0.0)
    for bad in (np.array([1.0, np.nan, np.inf, np.nan, 2.0]),        # a NaN against -inf
                np.array([1.0, np.inf, np.inf, np.nan, 2.0]),        # a sign flip of inf
                np.array([1.0, -np.inf, -np.inf, np.nan, 2.0]),
                np.array([1.0, -np.inf, np.inf, 3.0, 2.0]),          # a finite value against NaN
                np.array([np.nan, -np.inf, np.inf, np.nan, 2.0]),    # a NaN against a finite value
                np.array([1.0, -1e300, np.inf, np.nan, 2.0]),        # a finite value against -inf
                np.array([1.0 + 2e-9, -np.inf, np.inf, np.nan, 2.0])):
        with pytest.raises(AssertionError):
            assert_matches(bad, ref, None, 1e-9)


@pytest.mark.parametrize("V,field", [(6, "GT"), (16, "GP")])
def test_finaliser_prints_minus_infinity_as_the_oracle_does(eng, oracle, tmp_path, V, field):
    """dmx_write_single / dmx_write_doublet (with --write-pair) on the oracle's own arrays of a zero-row problem — a duplicated sample
    column, so exact ties meet -inf entries — against the oracle's four files."""
    g, sp = problem(eng, V, field, dup=(1, 2), seed=7000 + V)
    gz, _ = poison(g, "zero", np.random.default_rng(1), sp, no_sample0=True)
    bcs = [f"BC{(i * 7919) % 100003:06d}-1" for i in range(sp.n_cells)]
    sms = [f"S{j:02d}" for j in range(V)]
    ref = oracle.run_csr(oracle_csr(oracle, sp, bcs), sms, gz, oracle.Params(A2, 0.5, 0, 0, 0, True), str(tmp_path / "orc"))
    assert np.isneginf(ref.llksAB).any() and np.isneginf(ref.llks).any()
    fa = eng.FinalArgs(bcs, sms, A2, 0.5, sp.rd_totl, sp.rd_pass, sp.rd_uniq, np.diff(sp.cell_pair_off).astype(np.int32), 0, 0, 0, True)
    eng.write_single(fa, ref.llks, ref.llk0s, str(tmp_path / "o.single"))
    eng.write_doublet(fa, ref.llksAB, ref.llks00, str(tmp_path / "o"))
    for suf in ("single", "sing2", "best", "pair"):
        want = (tmp_path / f"orc.{suf}").read_bytes()
        assert (tmp_path / f"o.{suf}").read_bytes() == want, suf
        if suf in ("single", "pair"):
            assert len({ln.split(b"\t")[0] for ln in want.splitlines() if b"-inf" in ln}) >= 5
