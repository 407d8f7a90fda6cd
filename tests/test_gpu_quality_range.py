"""GPU (-m gpu): every K1 and K2 kernel family over the whole base-quality range of the C-ABI (0..127) and the read-count regimes of the
kernels, against the oracle.

The kernels choose their code path by base quality: gl_seed's pair tables need both reads below 64, its triple tables all three below
kTripleBq = 48, k_singlet_can / k_singlet_canp keep an LDS copy of the one-read table below kCtBq = 42, PhredHelper's error floor is 0.75
at q <= 1, and kSafeReads = 15 (the reciprocal-refined division) rests on err(127)/3 being the smallest factor one read can apply.
Each family is forced with the DMX_* experiment switches and its kernel name is asserted, so a dispatch change cannot skip a case
silently; each runs with the phase-1 final and seed tables at their defaults, off, and on at every depth.
Tolerance: STRICT within 1e-9 of the oracle everywhere; FAST within the same 1e-9 on the entries demuxlet prints or decides on
(test_gpu_parity.py::test_fast_mode_stays_within_tolerance)."""
import numpy as np
import pytest

from golden_util import printed_mask
from quality_mix import A2, FAMILIES, TABLES, family_problem, genotypes, kernel_named, mixed_depth_pileup, oracle_run, run_with_env

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def eng():
    from demuxlet_amd import build, capi, engine
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return engine


def max_diffs(out, ref, alphas, mode):
    proc = ref.processed.astype(bool)
    V, A = out["grid"].shape[1], len(alphas)
    mask = np.broadcast_to(printed_mask(V, A)[None] if mode == "fast" else np.ones((1, V, V, A), dtype=bool), out["grid"].shape) & proc[:, None, None, None]
    d = dict(llks=np.abs(out["llks"] - ref.llks).max(), llk0s=np.abs(out["llk0s"] - ref.llk0s).max(),
             grid=np.abs(out["grid"] - ref.llksAB)[mask].max() if mask.any() else 0.0,
             l00=np.abs(out["l00"][proc] - ref.llks00[proc]).max() if proc.any() else 0.0)
    return d


@pytest.mark.parametrize("quals", ["full", "edges", "max"])
@pytest.mark.parametrize("case,field,V,alphas,mode,env,k1,k2,dense,deep", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_kernel_family_against_oracle(eng, oracle, monkeypatch, case, field, V, alphas, mode, env, k1, k2, dense, deep, quals):
    g, sp = family_problem(eng, case, field, V, dense, deep, quals)
    bq = sp.reads & 0x7F
    assert (bq == 127).all() if quals == "max" else (bq.min() <= 1 and bq.max() >= 126)
    ref = oracle_run(oracle, sp, g, alphas)
    for tname, tenv in TABLES.items():
        out = run_with_env(eng, monkeypatch, g, sp, alphas, mode, {**env, **tenv})
        names = out["names"]
        assert names["singlet"].startswith(k1) and names["doublet"].startswith(k2), (tname, names)
        assert kernel_named(names["doublet"], k2), (tname, names)          # a whole K2 name is the whole name (k_doublet_a2u16 / its fall-back form)
        d = max_diffs(out, ref, alphas, mode)
        print(f"{case} {quals} {tname}: {names['singlet']} | {names['doublet']} | {names['certify']}: "
              + " ".join(f"{k} {v:.2e}" for k, v in d.items()))
        assert max(d.values()) < TOL, (tname, d)


@pytest.mark.parametrize("depths", [(14, 15, 16, 17), (40,), (250, 300, 400)], ids=["14-17", "40", "hundreds"])
@pytest.mark.parametrize("field,V", [("GT", 8), ("GP", 32), ("PL", 16), ("GT", 40)])
@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_depth_edges_at_quality_127(eng, oracle, monkeypatch, field, V, mode, depths):
    """Pairs of exactly 14..17 reads (both sides of kSafeReads = 15), 40 reads and a few hundred (u16 counts, the plain division), every
    read at quality 127, half the pairs all-ALT on a hom-REF source row (or all-REF on a hom-ALT one): the likelihoods shrink by
    err(127)/3 per read, the worst case of the division and of the final tables."""
    from demuxlet_amd import synth
    rng = np.random.default_rng(127000 + V + sum(depths) + (1 if mode == "fast" else 0))
    S, B = (120, 8) if max(depths) > 100 else (300, 16)
    raw = synth.make_raw_genotypes(rng, S, V)
    g = genotypes(eng, rng, raw.alleles, field)
    sp = mixed_depth_pileup(rng, raw.alleles, B, 0.25, quals="max", depths=depths, adversarial=0.5)
    assert set(np.unique(sp.pair_nrd)) <= set(depths) and (sp.reads & 0x7F == 127).all()
    ref = oracle_run(oracle, sp, g, A2)
    for tname, tenv in TABLES.items():
        out = run_with_env(eng, monkeypatch, g, sp, A2, mode, tenv)
        d = max_diffs(out, ref, A2, mode)
        print(f"{field} V={V} {mode} depths={depths} {tname}: {out['names']['singlet']} | {out['names']['doublet']}: "
              + " ".join(f"{k} {v:.2e}" for k, v in d.items()))
        assert max(d.values()) < TOL, (tname, d)
