"""GPU (-m gpu): the mirrored log of the STRICT unordered-pair doublet kernels.  k_doublet_a2u<k_doublet_a2u2> (dense pileups of 32 samples) and
k_doublet_a2u16 (16 samples) evaluate the log of the alpha-0.5 sum of entry [k][j] from the table entry, kd and w of entry [j][k]'s — the two sums are the same
nine terms in two orders — behind a guard on the two high words, and evaluate it whole, out of line, in a wavefront where the guard fails.  No pileup reaches
that path on purpose (a straddle has probability of order 1e-13 per pair), so each kernel has a form whose guard is compile-time false
(DMX_EXPERIMENTS=1 DMX_A2U_MIRROR_FALLBACK=1: k_doublet_a2u<k_doublet_a2u2_mirror_fallback>, k_doublet_a2u16_mirror_fallback), in which every such log takes it.

Problems as in test_gpu_a2u_two_barcodes.py (GP field, mixed depths per barcode and tile, the final-value table on): 32 samples, B in {1, 2, 3} barcodes x
S in {1, 33, 70} pairs, dense and sparse (the sparse layout launches k_doublet_a2u<4>, which keeps four independent logs per unit and has no fall-back form);
and 16 samples, B = 5, S = 33.  Per problem: grid, l00, llks, llk0s and the K3 records of the default run equal, bit for bit, the run with DMX_A2_NO_SYMU=1
(k_doublet_a2: ordered pairs, every log on its own — the independent yardstick) and the run with the fall-back form; both stay within 1e-9 of the oracle;
kernel_names shows the intended kernel in each run."""
import numpy as np
import pytest

from demuxlet_amd import synth
from quality_mix import genotypes, oracle_run, run_with_env
from test_gpu_a2u_two_barcodes import depths_of

pytestmark = pytest.mark.gpu
A2 = (0.0, 0.5)
FINALS = {"DMX_FINALS_ANY_DEPTH": "1"}
FALLBACK = {**FINALS, "DMX_A2U_MIRROR_FALLBACK": "1"}
OUTPUTS = ("grid", "l00", "llks", "llk0s")


def problem(eng, V, B, S, dense):
    """test_gpu_a2u_two_barcodes.problem for a panel of V samples, in one layout."""
    rng = np.random.default_rng(8900 + 1000 * V + 100 * B + S)
    raw = synth.make_raw_genotypes(rng, S, V)
    g = genotypes(eng, rng, raw.alleles, "GP")
    dosage = np.clip(raw.alleles, 0, 1).sum(axis=2)
    nrd = depths_of(rng, B, S).reshape(-1).astype(np.int64)
    cc, ss = np.repeat(np.arange(B), S), np.tile(np.arange(S), B)
    pr = np.repeat(np.arange(B * S), nrd)
    alt = rng.random(len(pr)) < dosage[ss[pr], cc[pr] % V] / 2.0
    bq = synth.draw_bq(rng, len(pr))
    hot = (nrd[pr] >= 4) & (rng.random(len(pr)) < 1 / 3)
    bq = np.where(hot, rng.integers(64, 128, size=len(pr)), bq).astype(np.uint8)
    reads = (bq | (alt.astype(np.uint8) << 7)).astype(np.uint8)
    cpo = (np.arange(B + 1) * S).astype(np.int64)
    totl = np.bincount(cc, weights=nrd, minlength=B).astype(np.int32)
    cro = np.concatenate([[0], np.cumsum(totl)]).astype(np.int64)
    truth = np.stack([np.arange(B) % V, np.full(B, -1)], axis=1).astype(np.int32)
    return g, synth.SynthPileup(B, S, cpo, cro, None if dense else ss.astype(np.int32), nrd.astype(np.uint8), reads, totl, totl.copy(), totl.copy(), truth)


@pytest.fixture(scope="module")
def eng():
    from demuxlet_amd import build, capi, engine
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return engine


def run(eng, monkeypatch, g, sp, env):
    for k in ("DMX_A2U_ONE_BARCODE", "DMX_A2U2_NO_DIAG", "DMX_A2U_MIRROR_FALLBACK"):   # (run_with_env clears them as well)
        monkeypatch.delenv(k, raising=False)
    return run_with_env(eng, monkeypatch, g, sp, A2, "strict", env)


def assert_same_bits(new, old, what):
    for n in OUTPUTS:
        assert new[n].tobytes() == old[n].tobytes(), f"{n}: {np.sum(new[n] != old[n])} values differ from {what}"
    for n in new["summ"].dtype.names:
        assert np.ascontiguousarray(new["summ"][n]).tobytes() == np.ascontiguousarray(old["summ"][n]).tobytes(), f"K3 record field {n} differs from {what}"


def assert_near_oracle(oracle, sp, g, got, what):
    ref = oracle_run(oracle, sp, g, A2)
    d = {"grid": np.abs(got["grid"] - ref.llksAB).max(), "l00": np.abs(got["l00"] - ref.llks00).max(),
         "llks": np.abs(got["llks"] - ref.llks).max(), "llk0s": np.abs(got["llk0s"] - ref.llk0s).max()}
    print(f"{what}: max |d| vs oracle {d}")
    assert max(d.values()) <= 1e-9, (what, d)


def check(eng, oracle, monkeypatch, V, B, S, dense, default_kernel, fallback_kernel):
    g, sp = problem(eng, V, B, S, dense)
    new = run(eng, monkeypatch, g, sp, FINALS)
    plain = run(eng, monkeypatch, g, sp, {**FINALS, "DMX_A2_NO_SYMU": "1"})
    slow = run(eng, monkeypatch, g, sp, FALLBACK)
    assert new["names"]["doublet"] == default_kernel or new["names"]["doublet"].startswith(default_kernel + "("), new["names"]
    assert plain["names"]["doublet"].startswith("k_doublet_a2<"), plain["names"]
    assert slow["names"]["doublet"] == fallback_kernel or slow["names"]["doublet"].startswith(fallback_kernel + "("), slow["names"]
    assert_same_bits(new, plain, "k_doublet_a2")
    assert_same_bits(new, slow, fallback_kernel)
    assert_near_oracle(oracle, sp, g, new, f"V={V} B={B} S={S} dense={dense} default")
    assert_near_oracle(oracle, sp, g, slow, f"V={V} B={B} S={S} dense={dense} fall-back")


CASES = [(B, S, dense) for dense in (True, False) for B in (1, 2, 3) for S in (1, 33, 70)]


@pytest.mark.parametrize("B,S,dense", CASES, ids=[f"B{B}-S{S}-{'dense' if d else 'sparse'}" for B, S, d in CASES])
def test_32_samples(eng, oracle, monkeypatch, B, S, dense):
    if dense:
        check(eng, oracle, monkeypatch, 32, B, S, True, "k_doublet_a2u<k_doublet_a2u2>", "k_doublet_a2u<k_doublet_a2u2_mirror_fallback>")
    else:                                        # k_doublet_a2u<4>: independent logs, the switch selects nothing
        check(eng, oracle, monkeypatch, 32, B, S, False, "k_doublet_a2u<4>", "k_doublet_a2u<4>")


def test_16_samples(eng, oracle, monkeypatch):
    check(eng, oracle, monkeypatch, 16, 5, 33, True, "k_doublet_a2u16", "k_doublet_a2u16_mirror_fallback")
