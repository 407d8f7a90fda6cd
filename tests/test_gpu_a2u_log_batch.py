"""GPU (-m gpu): phase 2 of the STRICT unordered-pair doublet kernels (k_doublet_a2u, k_doublet_a2u16) on ragged small problems.

Their phase-2 loop requests a unit's four log-table entries together, unit 1's k row behind unit 0's entries and the next pair's values
and rows behind unit 1's; the pair counter is a scalar.  Every barcode length at which that loop takes another shape is here: no pair at
all, a tile of one pair, one pair short of a tile, a full tile, a full tile and one pair, two full tiles and one pair (TP = 32).

Checked per problem: the unordered-pair kernel ran (kernel_names); grid, l00, llks, llk0s and the K3 records equal, bit for bit, a run
with DMX_A2_NO_SYMU=1 — k_doublet_a2, whose ordered-pair phase 2 evaluates the logs one after the other — and stay within 1e-9 of the
oracle.  The "depth" problems switch the final-value table on (DMX_FINALS_ANY_DEPTH=1): one barcode holds pairs of four and more reads
and base qualities of 64 and more (its tiles walk the read loop from the seed table), another only tabled pairs (the all-tabled
branch)."""
import numpy as np
import pytest

from demuxlet_amd import synth
from quality_mix import genotypes, oracle_run, run_with_env

pytestmark = pytest.mark.gpu
COUNTS = (0, 1, 31, 32, 33, 65)          # covered pairs per barcode (sparse layout)
S_SPARSE = 70
A2 = (0.0, 0.5)


def ragged_pileup(rng, alleles, counts, dense, depth=False):
    """A synth.SynthPileup over alleles [S][V][2], barcode c with counts[c] covered SNPs.  Dense layout: by the C-ABI's contract every barcode has S pairs
    (pair t is SNP t); the SNPs it does not cover are pairs of zero reads.  Pair depths 0..3, qualities 13..40 (every pair on the final-value table);
    with `depth`, the LONGEST barcode gets a third of its pairs at 4, 6 or 17 reads and a third of its reads at quality 64..127."""
    S, V, _ = alleles.shape
    B = len(counts)
    dosage = np.clip(alleles, 0, 1).sum(axis=2)
    deep_cell = int(np.argmax(counts))
    cc, ss, nrd = [], [], []
    for c, n in enumerate(counts):
        covered = np.sort(rng.choice(S, size=min(n, S), replace=False))
        d = rng.choice([0, 1, 2, 3], size=len(covered), p=[0.05, 0.45, 0.3, 0.2])
        if depth and c == deep_cell:
            d = np.where(rng.random(len(covered)) < 1 / 3, rng.choice([4, 6, 17], size=len(covered)), d)
        if dense:
            full = np.zeros(S, dtype=np.int64)
            full[covered] = d
            covered, d = np.arange(S), full
        cc.append(np.full(len(covered), c)); ss.append(covered); nrd.append(d)
    cc, ss, nrd = (np.concatenate(x).astype(np.int64) for x in (cc, ss, nrd))
    pr = np.repeat(np.arange(len(cc)), nrd)
    src = cc[pr] % V
    alt = rng.random(len(pr)) < dosage[ss[pr], src] / 2.0
    bq = synth.draw_bq(rng, len(pr))
    if depth:
        hot = (cc[pr] == deep_cell) & (rng.random(len(pr)) < 1 / 3)
        bq = np.where(hot, rng.integers(64, 128, size=len(pr)), bq).astype(np.uint8)
    reads = (bq | (alt.astype(np.uint8) << 7)).astype(np.uint8)
    cpo = np.concatenate([[0], np.cumsum(np.bincount(cc, minlength=B))]).astype(np.int64)
    totl = np.bincount(cc, weights=nrd, minlength=B).astype(np.int32)
    cro = np.concatenate([[0], np.cumsum(totl)]).astype(np.int64)
    truth = np.stack([np.arange(B) % V, np.full(B, -1)], axis=1).astype(np.int32)
    return synth.SynthPileup(B, S, cpo, cro, None if dense else ss.astype(np.int32), nrd.astype(np.uint8), reads, totl, totl.copy(), totl.copy(), truth)


@pytest.fixture(scope="module")
def eng():
    from demuxlet_amd import build, capi, engine
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return engine


def check(eng, oracle, monkeypatch, V, field, S, dense, depth, seed, symu_kernel, plain_kernel):
    rng = np.random.default_rng(seed)
    raw = synth.make_raw_genotypes(rng, S, V)
    g = genotypes(eng, rng, raw.alleles, field)
    sp = ragged_pileup(rng, raw.alleles, COUNTS, dense, depth)
    env = {"DMX_FINALS_ANY_DEPTH": "1"} if depth else {}
    new = run_with_env(eng, monkeypatch, g, sp, A2, "strict", env)
    old = run_with_env(eng, monkeypatch, g, sp, A2, "strict", {**env, "DMX_A2_NO_SYMU": "1"})
    assert new["names"]["doublet"].startswith(symu_kernel), new["names"]
    assert old["names"]["doublet"].startswith(plain_kernel), old["names"]
    for n in ("grid", "l00", "llks", "llk0s"):
        assert new[n].tobytes() == old[n].tobytes(), f"{n}: {np.sum(new[n] != old[n])} values differ from the ordered-pair kernel"
    for n in new["summ"].dtype.names:
        assert np.ascontiguousarray(new["summ"][n]).tobytes() == np.ascontiguousarray(old["summ"][n]).tobytes(), f"K3 record field {n}"
    ref = oracle_run(oracle, sp, g, A2)
    d = {"grid": np.abs(new["grid"] - ref.llksAB).max(), "l00": np.abs(new["l00"] - ref.llks00).max(),
         "llks": np.abs(new["llks"] - ref.llks).max(), "llk0s": np.abs(new["llk0s"] - ref.llk0s).max()}
    print(f"V={V} {field} S={S} dense={dense} depth={depth}: max |d| vs oracle {d}")
    assert max(d.values()) <= 1e-9, d


# sparse: the ragged pair counts over 70 SNPs; dense: every barcode has S pairs, so S itself walks the tile shapes
LAYOUTS = [("sparse", S_SPARSE, False), ("dense33", 33, True), ("dense65", 65, True)]


@pytest.mark.parametrize("layout,S,dense", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_a2u_ragged(eng, oracle, monkeypatch, layout, S, dense):
    check(eng, oracle, monkeypatch, 32, "GP", S, dense, False, 9100 + S, "k_doublet_a2u<", "k_doublet_a2<")


@pytest.mark.parametrize("layout,S,dense", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_a2u_ragged_with_depth(eng, oracle, monkeypatch, layout, S, dense):
    check(eng, oracle, monkeypatch, 32, "GP", S, dense, True, 9200 + S, "k_doublet_a2u<", "k_doublet_a2<")


@pytest.mark.parametrize("field", ["PL", "GP"])
@pytest.mark.parametrize("depth", [False, True], ids=["shallow", "depth"])
def test_a2u16_ragged(eng, oracle, monkeypatch, field, depth):
    check(eng, oracle, monkeypatch, 16, field, S_SPARSE, False, depth, 9300 + (field == "PL") + 10 * depth, "k_doublet_a2u16", "k_doublet_a2<")
