"""GPU (-m gpu): the headline kernel on the inputs it is shipped for.  k_doublet_a2u<k_doublet_a2u2> (STRICT, 32 soft-field samples, grid {0, 0.5}, DENSE
pileups: two barcodes per workgroup, k_doublet_diag_lo behind it) and its sibling forms, on problems of tests/quality_mix.py — the whole base-quality range,
every read-count regime, u16 read counts, adversarial allele patterns — where the three targeted files (test_gpu_a2u_two_barcodes.py, test_gpu_a2u_mirror.py,
test_gpu_a2u_log_batch.py) use shallow pairs with one-byte counts from host memory and the final-value table always on.

a. every form of the kernel and the two independent yardsticks (k_doublet_a2: ordered pairs; k_doublet_generic) on one problem, bit for bit, under each entry
   of quality_mix.TABLES; 32 and 16 samples.  Guards the shared products E = g_j x g_k and the u >= 496 diagonal units of a2u2_body.
b. pairs of 14..17, 40 and 250..400 reads at quality 127 (the dense twin of test_gpu_quality_range.py::test_depth_edges_at_quality_127).  Guards the
   per-wavefront table / loop choice of phase 1 at the depths where its division changes, and the header loads of two-byte counts.
c. a barcode's results do not depend on its partner in the workgroup: permuted barcodes, a lone last barcode, every barcode alone, twins.  Guards the
   lone-barcode path and the shared E products (and phase 1's per-wavefront choice: the partners' depths are as unlike as the tables allow).
d. the same pileup with wider read counts, from device memory, through run_singlet + run_doublet, under a longer genotype matrix.  Guards the header
   loading by nrd_width and the dense SNP index (pair p is SNP p whatever the matrix holds behind it).
Every run asserts the K2 kernel's name.  Tolerance against the oracle: the project's 1e-9 (STRICT).  (e., the job over ranges, is
test_gpu_parity.py::test_demuxlet_run_dense_headline_over_ranges.)"""
import dataclasses

import numpy as np
import pytest

from demuxlet_amd import synth
from quality_mix import A2, TABLES, genotypes, host_pileup, kernel_named, mixed_depth_pileup, oracle_run, run_with_env

pytestmark = pytest.mark.gpu
TOL = 1e-9
FINALS = {"DMX_FINALS_ANY_DEPTH": "1"}
OUTPUTS = ("grid", "l00", "llks", "llk0s")
K2_HEADLINE = "k_doublet_a2u<k_doublet_a2u2>"
# (label, switches, whole K2 name or prefix): the default form first
FORMS_32 = [("default", {}, K2_HEADLINE),
            ("whole_diag_behind", {"DMX_A2U2_NO_DIAG": "1"}, "k_doublet_a2u<k_doublet_a2u2_whole_diag_behind>"),
            ("mirror_fallback", {"DMX_A2U_MIRROR_FALLBACK": "1"}, "k_doublet_a2u<k_doublet_a2u2_mirror_fallback>"),
            ("one_barcode", {"DMX_A2U_ONE_BARCODE": "1"}, "k_doublet_a2u<4>"),
            ("ordered_pairs", {"DMX_A2_NO_SYMU": "1"}, "k_doublet_a2<"),
            ("generic", {"DMX_K2_GENERIC": "1"}, "k_doublet_generic<")]
FORMS_16 = [("default", {}, "k_doublet_a2u16"),
            ("mirror_fallback", {"DMX_A2U_MIRROR_FALLBACK": "1"}, "k_doublet_a2u16_mirror_fallback"),
            ("ordered_pairs", {"DMX_A2_NO_SYMU": "1"}, "k_doublet_a2<"),
            ("generic", {"DMX_K2_GENERIC": "1"}, "k_doublet_generic<")]


@pytest.fixture(scope="module")
def eng():
    from demuxlet_amd import build, capi, engine
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return engine


def run(eng, monkeypatch, g, sp, env, k2, **how):
    out = run_with_env(eng, monkeypatch, g, sp, A2, "strict", env, **how)
    assert kernel_named(out["names"]["doublet"], k2), (k2, env, out["names"])
    return out


def assert_same_bits(new, old, what, rows_new=None, rows_old=None):
    """The outputs of the barcodes rows_new of `new` and rows_old of `old` (all by default), field by field.  Of 32 samples the diagonal entries [j][j] come
    first, by the kernel that forms them behind / inside the headline kernel: j = 0..15 k_doublet_diag_lo, j = 16..31 a2u2_body's units u >= 496."""
    a = slice(None) if rows_new is None else np.asarray(rows_new)
    b = slice(None) if rows_old is None else np.asarray(rows_old)
    V = new["grid"].shape[1]
    if V == 32:
        j = np.arange(V)
        dn, do = new["grid"][a][:, j, j, :], old["grid"][b][:, j, j, :]
        assert dn[:, :16].tobytes() == do[:, :16].tobytes(), f"diagonal entries of j = 0..15 (k_doublet_diag_lo) differ from {what}"
        assert dn[:, 16:].tobytes() == do[:, 16:].tobytes(), f"diagonal entries of j = 16..31 (the kernel's own diagonal units) differ from {what}"
    for n in OUTPUTS:
        x, y = np.ascontiguousarray(new[n][a]), np.ascontiguousarray(old[n][b])
        assert x.tobytes() == y.tobytes(), f"{n}: {np.sum(x != y)} values differ from {what}"
    for n in new["summ"].dtype.names:
        assert np.ascontiguousarray(new["summ"][n][a]).tobytes() == np.ascontiguousarray(old["summ"][n][b]).tobytes(), f"K3 record field {n} differs from {what}"


def assert_near_oracle(ref, got, what, rows=None):
    r = slice(None) if rows is None else np.asarray(rows)
    d = {"grid": np.abs(got["grid"] - ref.llksAB[r]).max(), "l00": np.abs(got["l00"] - ref.llks00[r]).max(),
         "llks": np.abs(got["llks"] - ref.llks[r]).max(), "llk0s": np.abs(got["llk0s"] - ref.llk0s[r]).max()}
    print(f"{what}: {got['names']['doublet']}: max |d| vs oracle " + " ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert max(d.values()) < TOL, (what, d)


# ---- a. all forms on one problem

def check_all_forms(eng, oracle, monkeypatch, V, B, S, quals, forms):
    rng = np.random.default_rng(61000 + 100 * V + {"full": 0, "edges": 1, "max": 2}[quals])
    raw = synth.make_raw_genotypes(rng, S, V)
    g = genotypes(eng, rng, raw.alleles, "GP")
    sp = mixed_depth_pileup(rng, raw.alleles, B, 0.3, quals=quals, dense=True, deep=3)
    assert sp.pair_snp is None and sp.pair_nrd.dtype == np.uint16 and sp.pair_nrd.max() >= 256
    ref = oracle_run(oracle, sp, g, A2)
    for tname, tenv in TABLES.items():
        label0, env0, k2_0 = forms[0]
        first = run(eng, monkeypatch, g, sp, {**env0, **tenv}, k2_0)
        assert_near_oracle(ref, first, f"V={V} {quals} {tname} {label0}")
        for label, env, k2 in forms[1:]:
            other = run(eng, monkeypatch, g, sp, {**env, **tenv}, k2)
            assert_same_bits(first, other, f"{k2} ({label}, {tname})")


@pytest.mark.parametrize("quals", ["full", "edges", "max"])
def test_all_forms_give_the_same_bits_32_samples(eng, oracle, monkeypatch, quals):
    """B = 7: three two-barcode workgroups per slab and a lone last barcode; S = 70: two tiles and six pairs; three pairs of 256..300 reads."""
    check_all_forms(eng, oracle, monkeypatch, 32, 7, 70, quals, FORMS_32)


@pytest.mark.parametrize("quals", ["full", "edges", "max"])
def test_all_forms_give_the_same_bits_16_samples(eng, oracle, monkeypatch, quals):
    """B = 9: two workgroups of four barcodes and one of one."""
    check_all_forms(eng, oracle, monkeypatch, 16, 9, 70, quals, FORMS_16)


# ---- b. depth edges at quality 127, dense

@pytest.mark.parametrize("depths", [(14, 15, 16, 17), (40,), (250, 300, 400)], ids=["14-17", "40", "hundreds"])
@pytest.mark.parametrize("V,k2", [(32, K2_HEADLINE), (16, "k_doublet_a2u16")], ids=["GP-32", "GP-16"])
def test_depth_edges_at_quality_127_dense(eng, oracle, monkeypatch, V, k2, depths):
    """test_gpu_quality_range.py::test_depth_edges_at_quality_127 on a dense pileup: both sides of kSafeReads = 15, 40 reads, and a few hundred (two-byte
    counts), every read at quality 127, half the pairs adversarial.  S = 64: two full tiles; B = 5: a lone last barcode."""
    rng = np.random.default_rng(128000 + V + sum(depths))
    S, B = 64, 5
    raw = synth.make_raw_genotypes(rng, S, V)
    g = genotypes(eng, rng, raw.alleles, "GP")
    sp = mixed_depth_pileup(rng, raw.alleles, B, 0.25, quals="max", dense=True, depths=depths, adversarial=0.5)
    assert sp.pair_snp is None and set(np.unique(sp.pair_nrd)) <= set(depths) and (sp.reads & 0x7F == 127).all()
    assert sp.pair_nrd.dtype.itemsize == (2 if max(depths) > 255 else 1)
    ref = oracle_run(oracle, sp, g, A2)
    for tname, tenv in TABLES.items():
        out = run(eng, monkeypatch, g, sp, tenv, k2)
        assert_near_oracle(ref, out, f"GP V={V} dense depths={depths} {tname}")
        plain = run(eng, monkeypatch, g, sp, {**tenv, "DMX_A2_NO_SYMU": "1"}, "k_doublet_a2<")
        assert_same_bits(out, plain, f"k_doublet_a2 ({tname})")


# ---- c. partner independence

def unlike_barcodes(eng):
    """g [70][32][3] and eight barcodes (nrd [S], read bytes): the even ones all tabled (0..3 reads of base quality < 48 per pair, a few pairs without a read),
    the odd ones 17..40 reads per pair at base quality 64..127 — with the final-value table on, one wavefront of a workgroup's phase 1 takes the table for
    every tile while its partner's walks the read loop."""
    V, S, B = 32, 70, 8
    rng = np.random.default_rng(62000)
    raw = synth.make_raw_genotypes(rng, S, V)
    g = genotypes(eng, rng, raw.alleles, "GP")
    dosage = np.clip(raw.alleles, 0, 1).sum(axis=2)
    cells = []
    for c in range(B):
        nrd = rng.integers(17, 41, size=S) if c % 2 else rng.choice([0, 1, 2, 3], size=S, p=[0.1, 0.4, 0.3, 0.2])
        pr = np.repeat(np.arange(S), nrd)
        alt = rng.random(len(pr)) < dosage[pr, (5 * c + 3) % V] / 2.0
        bq = rng.integers(64, 128, size=len(pr)) if c % 2 else rng.integers(0, 48, size=len(pr))
        cells.append((nrd.astype(np.uint8), (bq | (alt.astype(np.int64) << 7)).astype(np.uint8)))
    return g, cells


def pileup_of(cells, S):
    """The dense pileup of the given barcodes, in the given order (pair_nrd and reads rebuilt per barcode)."""
    B = len(cells)
    totl = np.array([len(r) for _, r in cells], dtype=np.int32)
    return synth.SynthPileup(B, S, (np.arange(B + 1) * S).astype(np.int64), np.concatenate([[0], np.cumsum(totl)]).astype(np.int64), None,
                             np.concatenate([n for n, _ in cells]), np.concatenate([r for _, r in cells]).astype(np.uint8), totl, totl.copy(), totl.copy(),
                             np.full((B, 2), -1, dtype=np.int32))


def test_a_barcodes_bits_do_not_depend_on_its_partner(eng, oracle, monkeypatch):
    g, cells = unlike_barcodes(eng)
    S, B = g.shape[0], len(cells)
    whole_sp = pileup_of(cells, S)
    whole = run(eng, monkeypatch, g, whole_sp, FINALS, K2_HEADLINE)
    assert_near_oracle(oracle_run(oracle, whole_sp, g, A2), whole, "unlike partners")
    # every barcode beside another partner: workgroups (0, 2) (1, 3) (4, 6) (5, 7) instead of (0, 1) (2, 3) (4, 5) (6, 7) — barcodes of one pileup all have
    # S pairs, so the launch order is the barcode order
    perm = [0, 2, 1, 3, 4, 6, 5, 7]
    assert all(perm[i ^ 1] != (c ^ 1) for i, c in enumerate(perm))
    moved = run(eng, monkeypatch, g, pileup_of([cells[c] for c in perm], S), FINALS, K2_HEADLINE)
    assert_same_bits(moved, whole, "the run in the original barcode order", rows_old=perm)
    # the first seven: barcode 6 loses its partner and is walked twice
    seven = run(eng, monkeypatch, g, pileup_of(cells[:7], S), FINALS, K2_HEADLINE)
    assert_same_bits(seven, whole, "the run of all eight barcodes", rows_old=list(range(7)))
    # every barcode alone
    for c in range(B):
        alone = run(eng, monkeypatch, g, pileup_of([cells[c]], S), FINALS, K2_HEADLINE)
        assert_same_bits(alone, whole, f"barcode {c} in the run of all eight", rows_old=[c])
    # twins: a workgroup whose two barcodes are byte-identical (a tabled one, a deep one)
    for c in (0, 1):
        twins = run(eng, monkeypatch, g, pileup_of([cells[c], cells[c]], S), FINALS, K2_HEADLINE)
        assert_same_bits(twins, twins, "its twin in the same workgroup", rows_new=[0], rows_old=[1])
        assert_same_bits(twins, whole, f"barcode {c} in the run of all eight", rows_old=[c, c])


# ---- d. how the pileup arrives

@pytest.mark.parametrize("tables", ["tables_default", "tables_any_depth"])
def test_how_the_pileup_arrives_changes_no_bit(eng, oracle, monkeypatch, tables):
    import torch
    from demuxlet_amd import capi
    V, B, S, S_LONG = 32, 9, 70, 90
    env = TABLES[tables]
    rng = np.random.default_rng(63000)
    raw = synth.make_raw_genotypes(rng, S_LONG, V)
    g_long = genotypes(eng, rng, raw.alleles, "GP")
    g = np.ascontiguousarray(g_long[:S])
    sp = mixed_depth_pileup(rng, raw.alleles[:S], B, 0.3, quals="full", dense=True)
    assert sp.pair_snp is None and sp.pair_nrd.dtype == np.uint8 and sp.n_snps == S
    want = run(eng, monkeypatch, g, sp, env, K2_HEADLINE)
    ref = oracle_run(oracle, sp, g, A2)
    assert_near_oracle(ref, want, f"host, one-byte counts, {tables}")
    # read counts of two and four bytes
    for dt in (np.uint16, np.uint32):
        wide = dataclasses.replace(sp, pair_nrd=sp.pair_nrd.astype(dt))
        assert_same_bits(run(eng, monkeypatch, g, wide, env, K2_HEADLINE), want, f"the one-byte counts ({np.dtype(dt).name})")
    # the five arrays in device memory: a view of the caller's arrays
    pl = host_pileup(eng, sp)
    hs = pl.as_struct()
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(pl, k))).to(dev) for k in ("cell_pair_off", "cell_read_off", "pair_nrd", "reads")}
    ds = capi.Pileup(B, S, hs.n_pairs, hs.n_reads, t["cell_pair_off"].data_ptr(), t["cell_read_off"].data_ptr(), None, t["pair_nrd"].data_ptr(),
                     pl.pair_nrd.dtype.itemsize, capi.DMX_MEM_DEVICE, t["reads"].data_ptr(), pl.rd_totl.ctypes.data, pl.rd_pass.ctypes.data,
                     pl.rd_uniq.ctypes.data)

    from_device = run(eng, monkeypatch, g, sp, env, K2_HEADLINE, stage=lambda e: e.set_pileup_struct(ds, keep=(t, pl)))
    assert_same_bits(from_device, want, "the host pileup (device-resident arrays)")
    # run_singlet, then run_doublet
    assert_same_bits(run(eng, monkeypatch, g, sp, env, K2_HEADLINE, split=True), want, "dmx_engine_run (run_singlet + run_doublet)")
    # a genotype matrix of 90 SNPs under the pileup of 70: pair p is still SNP p (against the oracle on the first 70 rows and a host run of its own)
    longer = run(eng, monkeypatch, g_long, sp, env, K2_HEADLINE)
    assert_near_oracle(ref, longer, f"genotype matrix of {S_LONG} SNPs, {tables}")       # (ref: the oracle on g = g_long[:S])
    truncated = run(eng, monkeypatch, np.array(g_long[:S]), sp, env, K2_HEADLINE)
    assert_same_bits(longer, truncated, f"the run with the matrix truncated to {S} SNPs")
