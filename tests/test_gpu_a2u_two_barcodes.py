"""GPU (-m gpu): k_doublet_a2u2 — the STRICT unordered-pair doublet kernel of DENSE pileups (32 soft-field samples, default grid, safe rows), in which a
workgroup owns two barcodes and one slab of the 496 unordered pairs and forms the products g_j[l] g_k[m] of a unit once for both barcodes.  It is a form of the
unordered-pair kernel: kernel_names reports k_doublet_a2u<k_doublet_a2u2> (k_doublet_a2u<4> is the one-barcode kernel).

Shapes: B in {1, 2, 3, 5} barcodes — a lone barcode (its workgroup walks it twice and stores once), a full workgroup, an odd count, three workgroups
per slab — and S in {1, 31, 32, 33, 70} SNPs = pairs per barcode: one pair, one pair short of a tile, a full tile, a tile and a pair, two tiles and a
partial one (tiles of 32 pairs).  Read depths are mixed per (barcode, tile): tile t of barcode c holds a pair of 5, 9 or 17 reads, a third of them of base
quality 64..127, when c + t is even (with the final-value table on, that barcode's wavefront walks the read loop for the tile while the other barcode's takes
the table), and only pairs of 0..3 tabled reads otherwise; every barcode has a pair without any read (the one-pair problems: the odd barcodes' only pair).

Checked per problem, with the final-value table on (DMX_FINALS_ANY_DEPTH=1: small jobs do not build it otherwise): the kernel ran (kernel_names); grid,
llks00, the singlet arrays and the K3 records equal, bit for bit, the run with DMX_A2U_ONE_BARCODE=1 (k_doublet_a2u: one barcode per workgroup, two units per
thread) and the run with DMX_A2_NO_SYMU=1 (k_doublet_a2: ordered pairs), and stay within 1e-9 of the oracle; the same pairs in the sparse layout (an explicit
SNP id per pair) still launch k_doublet_a2u and give the same bits.  One problem also runs phase 1's other two sources (the seed table alone, the nine-value
read loop)."""
import numpy as np
import pytest

from demuxlet_amd import synth
from quality_mix import genotypes, oracle_run, run_with_env

pytestmark = pytest.mark.gpu
A2 = (0.0, 0.5)
V = 32
BS = (1, 2, 3, 5)
SS = (1, 31, 32, 33, 70)
TP = 32                                          # pairs per tile
FINALS = {"DMX_FINALS_ANY_DEPTH": "1"}
OUTPUTS = ("grid", "l00", "llks", "llk0s")


def depths_of(rng, B, S):
    """[B][S] read counts: see the module docstring."""
    d = rng.choice([1, 2, 3], size=(B, S), p=[0.5, 0.3, 0.2])
    for c in range(B):
        for t in range((S + TP - 1) // TP):
            lo, hi = t * TP, min(S, (t + 1) * TP)
            if (c + t) % 2 == 0:
                d[c, lo + min(5 + c, hi - lo - 1)] = (5, 9, 17)[(c + t) // 2 % 3]
        if S > 1:
            d[c, c % 2] = 0
        elif c % 2:
            d[c, 0] = 0
    return d


def problem(eng, B, S):
    rng = np.random.default_rng(8800 + 100 * B + S)
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

    def pileup(dense):
        return synth.SynthPileup(B, S, cpo, cro, None if dense else ss.astype(np.int32), nrd.astype(np.uint8), reads, totl, totl.copy(), totl.copy(), truth)

    return g, pileup(True), pileup(False)


@pytest.fixture(scope="module")
def eng():
    from demuxlet_amd import build, capi, engine
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return engine


def run(eng, monkeypatch, g, sp, env):
    for k in ("DMX_A2U_ONE_BARCODE", "DMX_A2U2_NO_DIAG"):         # (run_with_env clears them as well)
        monkeypatch.delenv(k, raising=False)
    return run_with_env(eng, monkeypatch, g, sp, A2, "strict", env)


def two_barcode_kernel(names):
    """kernel_names reports k_doublet_a2u2: the two-barcode kernel is the form k_doublet_a2u<k_doublet_a2u2...> of the unordered-pair kernel."""
    return names["doublet"].startswith("k_doublet_a2u<") and "k_doublet_a2u2" in names["doublet"]


def one_barcode_kernel(names):
    return names["doublet"].startswith("k_doublet_a2u<") and "k_doublet_a2u2" not in names["doublet"]


_SHARED = {}                                     # (B, S) -> the problem and the two-barcode kernel's outputs: computed once, never modified


def shared(eng, monkeypatch, B, S):
    if (B, S) not in _SHARED:
        g, dense, sparse = problem(eng, B, S)
        new = run(eng, monkeypatch, g, dense, FINALS)
        assert two_barcode_kernel(new["names"]), new["names"]
        _SHARED[(B, S)] = (g, dense, sparse, new)
    return _SHARED[(B, S)]


def assert_same_bits(new, old, what):
    # the diagonal entries [j][j] first, by the kernel that forms them: j = 0..15 k_doublet_diag_lo, j = 16..31 k_doublet_a2u2's last sixteen slots of slab 1
    j = np.arange(V)
    dn, do = new["grid"][:, j, j, :], old["grid"][:, j, j, :]
    assert dn[:, :16].tobytes() == do[:, :16].tobytes(), f"diagonal entries of j = 0..15 (k_doublet_diag_lo) differ from {what}"
    assert dn[:, 16:].tobytes() == do[:, 16:].tobytes(), f"diagonal entries of j = 16..31 (k_doublet_a2u2's diagonal units) differ from {what}"
    for n in OUTPUTS:
        assert new[n].tobytes() == old[n].tobytes(), f"{n}: {np.sum(new[n] != old[n])} values differ from {what}"
    for n in new["summ"].dtype.names:
        assert np.ascontiguousarray(new["summ"][n]).tobytes() == np.ascontiguousarray(old["summ"][n]).tobytes(), f"K3 record field {n} differs from {what}"


CASES = [(B, S) for B in BS for S in SS]
IDS = [f"B{B}-S{S}" for B, S in CASES]


@pytest.mark.parametrize("B,S", CASES, ids=IDS)
def test_two_barcodes_give_the_one_barcode_kernels_bits(eng, monkeypatch, B, S):
    g, dense, _, new = shared(eng, monkeypatch, B, S)
    one = run(eng, monkeypatch, g, dense, {**FINALS, "DMX_A2U_ONE_BARCODE": "1"})
    assert one_barcode_kernel(one["names"]), one["names"]
    assert_same_bits(new, one, "k_doublet_a2u")
    plain = run(eng, monkeypatch, g, dense, {**FINALS, "DMX_A2_NO_SYMU": "1"})
    assert plain["names"]["doublet"].startswith("k_doublet_a2<"), plain["names"]
    assert_same_bits(new, plain, "k_doublet_a2")


@pytest.mark.parametrize("B,S", CASES, ids=IDS)
def test_two_barcodes_agree_with_the_oracle(eng, oracle, monkeypatch, B, S):
    g, dense, _, new = shared(eng, monkeypatch, B, S)
    ref = oracle_run(oracle, dense, g, A2)
    d = {"grid": np.abs(new["grid"] - ref.llksAB).max(), "l00": np.abs(new["l00"] - ref.llks00).max(),
         "llks": np.abs(new["llks"] - ref.llks).max(), "llk0s": np.abs(new["llk0s"] - ref.llk0s).max()}
    print(f"B={B} S={S}: max |d| vs oracle {d}")
    assert max(d.values()) <= 1e-9, d


@pytest.mark.parametrize("B,S", CASES, ids=IDS)
def test_sparse_layout_keeps_the_one_barcode_kernel(eng, monkeypatch, B, S):
    g, _, sparse, new = shared(eng, monkeypatch, B, S)
    got = run(eng, monkeypatch, g, sparse, FINALS)
    assert one_barcode_kernel(got["names"]), got["names"]
    assert_same_bits(new, got, "k_doublet_a2u on the sparse layout")


@pytest.mark.parametrize("env", [{}, {"DMX_A2_NO_SEEDS": "1", "DMX_A2_NO_FINALS": "1"}, {**FINALS, "DMX_A2U2_NO_DIAG": "1"}],
                         ids=["seed_table", "nine_value_loop", "whole_diagonal_behind"])
def test_phase_one_sources_and_diagonal_forms_give_the_same_bits(eng, monkeypatch, env):
    """Phase 1 from the seed table alone and from the nine-value read loop; and the kernel without its diagonal units (DMX_A2U2_NO_DIAG=1: k_doublet_diag behind it
    owns all 32 diagonal entries)."""
    g, dense, _, new = shared(eng, monkeypatch, 3, 70)
    got = run(eng, monkeypatch, g, dense, env)
    assert two_barcode_kernel(got["names"]), got["names"]
    assert_same_bits(new, got, f"k_doublet_a2u2 with the final-value table ({env})")
