"""GPU (-m gpu): the HIP path, through the C-ABI, against (a) the reference's own outputs (tests/golden) and (b) the
oracle on seeded problems, plus the edge cases of the domain.

Tolerance (BASELINE.json north_star): log-likelihoods within 1e-9 ABSOLUTE of the reference; .best assignments identical.
Bit-exact where the work is integer/index: cell ids, counters, argmax indices, the staged pileup."""
import numpy as np
import pytest

from golden_util import CASES, Golden

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


def build_store(eng, pb):
    st = eng.Store()
    for _ in range(pb.n_snps):
        st.add_snp()
    ev = pb.events
    for e in range(len(ev.barcode)):
        c = st.add_cell(ev.barcode[e])
        if ev.newread[e]:
            st.count_read(c)
        if ev.snp[e] >= 0:
            st.add_read(int(ev.snp[e]), c, ev.umi[e], int(ev.allele[e]), int(ev.bq[e]))
    return st


def run_engine(eng, pl, g, alphas, prior, doublet=True):
    e = eng.Engine(g.shape[1], alphas, prior)
    e.set_genotypes(g)
    e.set_pileup(pl)
    e.run_singlet()
    llks, llk0s = e.get_singlet()
    out = dict(llks=llks, llk0s=llk0s)
    if doublet:
        e.run_doublet()
        grid, l00, summ = e.get_doublet()
        out.update(grid=grid, l00=l00, summ=summ)
    e.close()
    return out


@pytest.mark.parametrize("name", CASES)
def test_golden_raw_arrays(eng, oracle, name):
    gd = Golden(name)
    pb = gd.problem(oracle)
    st = build_store(eng, pb)
    pl = st.freeze()
    out = run_engine(eng, pl, gd.g, gd.alphas, gd.doublet_prior)
    proc = gd.z["ref_processed"].astype(bool)
    d1 = np.abs(out["llks"] - gd.z["ref_llks"]).max()
    d0 = np.abs(out["llk0s"] - gd.z["ref_llk0s"]).max()
    # the reference only fills the grid of cells that pass the filters; the engine fills every cell
    dg = np.abs(out["grid"][proc] - gd.z["ref_llksAB"][proc]).max()
    d00 = np.abs(out["l00"][proc] - gd.z["ref_llks00"][proc]).max()
    print(f"{name}: max|d| llks={d1:.2e} llk0s={d0:.2e} grid={dg:.2e} llks00={d00:.2e}")
    assert max(d1, d0, dg, d00) < TOL

@pytest.mark.parametrize("name", CASES)
def test_golden_files_end_to_end_fast_mode(eng, oracle, name, tmp_path):
    """The same twelve jobs in DMX_MODE_FAST (`demuxlet --fast`), against the REFERENCE's files: every string field identical
    (barcodes, sample ids, BEST calls, the order of the two samples of a doublet) and — on these deterministic fixtures — every
    printed number too (FAST moves a log-likelihood by ~1e-11: no printed digit flips; asserted, as in the STRICT twin)."""
    from demuxlet_amd import capi
    gd = Golden(name)
    pb = gd.problem(oracle)
    st = build_store(eng, pb)
    eng.demuxlet_run(st, gd.g, gd.sample_ids, gd.alphas, str(tmp_path / "o"), gd.doublet_prior, gd.min_total, gd.min_uniq,
                     gd.min_snp, gd.write_pair, arbiter=True, n_gpus=2, mode=capi.DMX_MODE_FAST)
    n_text_diff = 0
    for suf, ref in gd.files.items():
        got = (tmp_path / f"o.{suf}").read_text().splitlines()
        want = ref.decode().splitlines()
        assert len(got) == len(want), suf
        assert got[0] == want[0]
        for a, b in zip(got[1:], want[1:]):
            fa, fb = a.split("\t"), b.split("\t")
            assert len(fa) == len(fb)
            for x, y in zip(fa, fb):
                try:
                    fx, fy = float(x), float(y)
                except ValueError:
                    assert x == y, (suf, a, b)
                    continue
                if x != y:
                    n_text_diff += 1
                    assert abs(fx - fy) <= 1e-3 * max(1e-3, abs(fy)) + 1.01e-4, (suf, a, b)
    print(f"{name}: FAST end to end, {n_text_diff} printed numbers differ in the last digit")
    assert n_text_diff == 0



@pytest.mark.parametrize("n_gpus,range_bytes", [(1, 0), (3, 0), (1, 3000), (2, 20000)])
@pytest.mark.parametrize("name", CASES)
def test_golden_files_end_to_end(eng, oracle, name, n_gpus, range_bytes, tmp_path, monkeypatch):
    """Store -> engine -> finaliser with the tie arbiter == the reference's four files.  n_gpus = 3 shards the sorted
    barcodes over three engines (all on device 0 on a 1-GPU box: same code path as three devices) and must not change a byte;
    DMX_RANGE_BYTES forces the doublet grid through the engines in many small ranges (several waves, rows appended range
    by range while the next wave computes), which must not change a byte either."""
    if range_bytes:
        monkeypatch.setenv("DMX_RANGE_BYTES", str(range_bytes))
    else:
        monkeypatch.delenv("DMX_RANGE_BYTES", raising=False)
    gd = Golden(name)
    pb = gd.problem(oracle)
    st = build_store(eng, pb)
    eng.demuxlet_run(st, gd.g, gd.sample_ids, gd.alphas, str(tmp_path / "o"), gd.doublet_prior, gd.min_total, gd.min_uniq,
                     gd.min_snp, gd.write_pair, arbiter=True, n_gpus=n_gpus)
    for suf, ref in gd.files.items():
        got = (tmp_path / f"o.{suf}").read_text().splitlines()
        want = ref.decode().splitlines()
        assert len(got) == len(want), suf
        assert got[0] == want[0]
        n_text_diff = 0
        for a, b in zip(got[1:], want[1:]):
            fa, fb = a.split("\t"), b.split("\t")
            assert len(fa) == len(fb)
            for x, y in zip(fa, fb):
                try:
                    fx, fy = float(x), float(y)
                except ValueError:
                    assert x == y, (suf, a, b)          # barcodes, sample ids, BEST strings: exact
                    continue
                if x != y:
                    n_text_diff += 1
                    assert abs(fx - fy) <= 1e-3 * max(1e-3, abs(fy)) + 1.01e-4, (suf, a, b)   # last printed digit only
        # deterministic inputs, deterministic kernels: on these ten fixtures STRICT + arbiter reproduces the reference's files
        # byte for byte (what DESIGN.md claims); if a printed digit ever flips, this is where it shows
        assert n_text_diff == 0 and (tmp_path / f"o.{suf}").read_bytes() == ref, (name, suf, n_text_diff)
        if suf == "best":
            assert [r.split("\t")[5] for r in got] == [r.split("\t")[5] for r in want]
    assert (tmp_path / "o.pair").exists() == gd.write_pair


def summary_from_grid(grid, l00, alphas, prior):
    """What K3 must return, computed with the reference's scans on the host (numpy), for index-exact comparison."""
    V, _, A = grid.shape
    mx = grid.max()
    sing = grid[:, 0, 0]
    i1 = int(np.argmax(sing))
    rest = sing.copy(); rest[i1] = -np.inf
    i2 = int(np.argmax(rest)) if V > 1 else -1
    best, arg = -1e300, (-1, -1, -1)
    for j in range(V):
        for k in range(V):
            if j == k: continue
            for n in range(1, A):
                if best < grid[j, k, n]:
                    best, arg = grid[j, k, n], (j, k, n)
    ss = sum(np.exp(grid[j, 0, 0] - mx) * (1 - prior) / V for j in range(V))
    sd = sum(np.exp(grid[j, k, n] - mx) * prior / V / (V - 1) / (A - 1) / (2.0 if alphas[n] == 0.5 else 1.0)
             for j in range(V) for k in range(V) if j != k for n in range(1, A))
    return mx, ss, sd, i1, i2, arg


@pytest.mark.parametrize("name", ["gt_v4_a2_pair", "pl_v32_a3", "gt_v3_alpha_quirk"])
def test_device_reduce_matches_host_scans(eng, oracle, name):
    gd = Golden(name)
    st = build_store(eng, gd.problem(oracle))
    pl = st.freeze()
    out = run_engine(eng, pl, gd.g, gd.alphas, gd.doublet_prior)
    for c in range(pl.n_cells):
        s = out["summ"][c]
        assert s["n_pairs"] == pl.n_snp_per_cell[c]
        if pl.n_snp_per_cell[c] == 0:
            continue
        mx, ss, sd, i1, i2, (j, k, n) = summary_from_grid(out["grid"][c], out["l00"][c], gd.alphas, gd.doublet_prior)
        assert s["max_llk"] == mx
        assert (s["i_sing1"], s["i_sing2"], s["j_best"], s["k_best"], s["n_best"]) == (i1, i2, j, k, n)
        assert s["llk12"] == out["grid"][c][j, k, n] and s["llk10"] == out["grid"][c][j, 0, n] and s["llk20"] == out["grid"][c][k, 0, n]
        assert s["llk00_0"] == out["l00"][c][0] and s["llk00_best"] == out["l00"][c][n]
        assert abs(s["sum_single"] - ss) <= 1e-12 * ss and abs(s["sum_double"] - sd) <= 1e-12 * max(sd, 1e-300)


def synth_problem(seed, B, S, V, delta, rbar, dense=False, field="GT"):
    from demuxlet_amd import synth
    rng = np.random.default_rng(seed)
    raw = synth.make_raw_genotypes(rng, S, V)
    return rng, raw, synth.make_pileup(rng, raw.alleles, B, delta, rbar, dense_layout=dense, doublet_rate=0.3)


def oracle_from_pileup(oracle, sp, g, alphas, prior, singlet_only=False):
    """Feed a C-ABI pileup to the oracle (words rebuilt from the packed read bytes)."""
    al = (sp.reads >> 7).astype(np.uint32)
    bq = (sp.reads & 0x7F).astype(np.uint32)
    words = (al << 24) | (bq << 16) | 1
    pair_snp = sp.pair_snp if sp.pair_snp is not None else np.tile(np.arange(sp.n_snps, dtype=np.int32), sp.n_cells)
    pair_off = np.concatenate([[0], np.cumsum(sp.pair_nrd.astype(np.int64))])
    csr = oracle.Csr([f"c{i:06d}" for i in range(sp.n_cells)], sp.cell_pair_off, pair_snp, pair_off, words.astype(np.uint32),
                     sp.rd_totl, sp.rd_pass, sp.rd_uniq)
    return oracle.run_csr(csr, [f"s{j}" for j in range(g.shape[1])], g, oracle.Params(tuple(alphas), prior), None, singlet_only)


def host_pileup(eng, sp):
    return eng.HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads,
                          sp.rd_totl, sp.rd_pass, sp.rd_uniq)


@pytest.mark.parametrize("B,S,V,alphas,delta,rbar,dense", [
    (37, 700, 2, (0.0, 0.5), 0.2, 1.5, False),          # tutorial-like V=2
    (300, 257, 8, (0.0, 0.5), 1.0, 1.25, True),         # dense layout (config 2 shape, small)
    (40, 3000, 16, (0.0, 0.5), 0.05, 2.0, False),       # sparse (config 5 shape, small)
    (9, 400, 33, (0.0, 0.3, 0.5), 0.3, 1.25, False),    # V not a multiple of anything, A=3
    (5, 300, 65, (0.0, 0.5), 0.3, 1.25, False),         # V just above a chunk/register boundary
    (20, 500, 5, (0.0, 0.1, 0.2, 0.3, 0.5), 0.3, 4.0, False),   # A=5 (padded to 8 lanes per pair)
    (4, 200, 100, (0.0, 0.5), 0.3, 1.25, False),        # wide panel: 20 002 accumulators per cell -> 3 slabs of the generic K2
    (3, 150, 70, (0.0, 0.1, 0.25, 0.4, 0.5), 0.3, 1.5, False),   # V=70 x A=5: 24 505 accumulators, slabs + padded alphas
    (2, 120, 200, (0.0, 0.5), 0.4, 1.25, True),         # V=200 (dense): general K1 with 25 chunks, 10 slabs in K2
    (2, 60, 600, (0.0, 0.5), 0.4, 1.25, False),         # V=600: K1 in two sample slabs (75 chunks > 56), class K2 in 100 j-slabs
])
def test_seeded_problems_against_oracle(eng, oracle, B, S, V, alphas, delta, rbar, dense):
    rng, raw, sp = synth_problem(1000 + B + V, B, S, V, delta, rbar, dense)
    g = np.stack([oracle.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    ref = oracle_from_pileup(oracle, sp, g, alphas, 0.5)
    out = run_engine(eng, host_pileup(eng, sp), g, alphas, 0.5)
    d = [np.abs(out["llks"] - ref.llks).max(), np.abs(out["llk0s"] - ref.llk0s).max()]
    proc = ref.processed.astype(bool)
    d += [np.abs(out["grid"][proc] - ref.llksAB[proc]).max(), np.abs(out["l00"][proc] - ref.llks00[proc]).max()]
    print(f"B={B} S={S} V={V} A={len(alphas)}: max|d| = " + " ".join(f"{x:.2e}" for x in d))
    assert max(d) < TOL


def test_full_snp_depth_few_cells(eng, oracle):
    """BASELINE config-2/3 depth (S = 50 000 SNPs per cell, dense) on a handful of cells: |LLK| reaches 1e5, where only
    the reference's accumulation ORDER keeps the difference below 1e-9."""
    rng, raw, sp = synth_problem(77, 6, 50000, 8, 1.0, 1.25, True)
    g = np.stack([oracle.geno_from_gt(raw.alleles[s], 0.01) for s in range(50000)])
    ref = oracle_from_pileup(oracle, sp, g, (0.0, 0.5), 0.5)
    out = run_engine(eng, host_pileup(eng, sp), g, (0.0, 0.5), 0.5)
    d = max(np.abs(out["llks"] - ref.llks).max(), np.abs(out["llk0s"] - ref.llk0s).max(), np.abs(out["grid"] - ref.llksAB).max(),
            np.abs(out["l00"] - ref.llks00).max())
    print(f"S=50000: |LLK| up to {np.abs(ref.llksAB).max():.3e}, max|d| = {d:.2e}")
    assert d < TOL


def test_edge_cases(eng, oracle):
    from demuxlet_amd import capi
    V, S = 4, 50
    rng = np.random.default_rng(3)
    g = rng.dirichlet([1, 1, 1], size=(S, V)).astype(np.float32)
    # (1) a cell with no pairs, a pair with zero stored reads (only allele-2 reads), a pair with 300 reads (u16 counts)
    cell_pair_off = np.array([0, 0, 2, 3], dtype=np.int64)
    pair_snp = np.array([3, 7, 49], dtype=np.int32)
    pair_nrd = np.array([0, 300, 2], dtype=np.uint16)
    reads = rng.integers(13, 41, size=302).astype(np.uint8) | (rng.integers(0, 2, size=302).astype(np.uint8) << 7)
    cell_read_off = np.array([0, 0, 300, 302], dtype=np.int64)
    z = np.zeros(3, dtype=np.int32)
    pl = eng.HostPileup(3, S, cell_pair_off, cell_read_off, pair_snp, pair_nrd, reads, z, z, z)
    out = run_engine(eng, pl, g, (0.0, 0.5), 0.5)

    class SP: pass
    sp = SP(); sp.reads = reads; sp.pair_snp = pair_snp; sp.n_snps = S; sp.n_cells = 3; sp.pair_nrd = pair_nrd
    sp.cell_pair_off = cell_pair_off; sp.rd_totl = sp.rd_pass = sp.rd_uniq = z
    ref = oracle_from_pileup(oracle, sp, g, (0.0, 0.5), 0.5)
    assert np.all(out["llks"][0] == 0) and out["llk0s"][0] == 0 and np.all(out["grid"][0] == 0)
    assert np.abs(out["llks"] - ref.llks).max() < TOL and np.abs(out["grid"][1:] - ref.llksAB[1:]).max() < TOL
    assert out["summ"]["n_pairs"].tolist() == [0, 2, 1]
    # (2) empty pileup
    pl0 = eng.HostPileup(0, S, np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32),
                         np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), z[:0], z[:0], z[:0])
    out0 = run_engine(eng, pl0, g, (0.0, 0.5), 0.5)
    assert out0["llks"].shape == (0, V) and out0["grid"].shape == (0, V, V, 2)
    # (3) error behaviour: doublet stage needs V >= 2 and A >= 2 (division by zero / index -1 in the reference, :731,:821)
    e = eng.Engine(1, (0.0, 0.5))
    e.set_genotypes(g[:, :1]); e.set_pileup(pl)
    e.run_singlet()
    with pytest.raises(capi.DmxError):
        e.run_doublet()
    e.close()
    # (4) out-of-range SNP id is refused at staging, not dereferenced on the device
    bad = eng.HostPileup(3, S, cell_pair_off, cell_read_off, np.array([3, 7, 50], dtype=np.int32), pair_nrd, reads, z, z, z)
    e = eng.Engine(V, (0.0, 0.5)); e.set_genotypes(g)
    with pytest.raises(capi.DmxError):
        e.set_pileup(bad)
    e.close()


def test_size_independent_properties(eng):
    """Properties that need no oracle (usable at any size): (i) permuting the cells permutes the results bit-for-bit;
    (ii) alpha=0.5 grid is symmetric to ~1e-11; (iii) duplicating the sample panel duplicates the singlet columns;
    (iv) llksAB[j][j][n] does not depend on n's alpha... only for l==m terms — not a property; skipped."""
    from demuxlet_amd import synth
    rng = np.random.default_rng(9)
    S, V, B = 600, 6, 64
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    sp = synth.make_pileup(rng, raw.alleles, B, 0.2, 1.5)
    out = run_engine(eng, host_pileup(eng, sp), g, (0.0, 0.5), 0.5)
    # (i) reverse the cell order
    order = np.arange(B)[::-1]
    npair = np.diff(sp.cell_pair_off); nread = np.diff(sp.cell_read_off)
    pair_idx = np.concatenate([np.arange(sp.cell_pair_off[c], sp.cell_pair_off[c + 1]) for c in order])
    read_idx = np.concatenate([np.arange(sp.cell_read_off[c], sp.cell_read_off[c + 1]) for c in order])
    sp2 = eng.HostPileup(B, S, np.concatenate([[0], np.cumsum(npair[order])]), np.concatenate([[0], np.cumsum(nread[order])]),
                         sp.pair_snp[pair_idx], sp.pair_nrd[pair_idx], sp.reads[read_idx], sp.rd_totl[order], sp.rd_pass[order],
                         sp.rd_uniq[order])
    out2 = run_engine(eng, sp2, g, (0.0, 0.5), 0.5)
    assert np.array_equal(out2["llks"], out["llks"][order]) and np.array_equal(out2["grid"], out["grid"][order])
    # (ii)
    assert np.abs(out["grid"][..., 1] - out["grid"][..., 1].transpose(0, 2, 1)).max() < 1e-9
    # (iii)
    g2 = np.concatenate([g, g], axis=1)
    out3 = run_engine(eng, host_pileup(eng, sp), g2, (0.0, 0.5), 0.5, doublet=False)
    assert np.array_equal(out3["llks"][:, :V], out["llks"]) and np.array_equal(out3["llks"][:, V:], out["llks"])


@pytest.mark.parametrize("name", ["gt_v4_a2_pair", "gp_v8_a2_minsnp", "gt_v5_dense", "pl_v32_a3"])
def test_records_path_end_to_end(eng, oracle, name, tmp_path):
    """The multi-GPU record path on one GPU: engine -> (llks, llk0s, sing, llks00, K3 summary) -> summary writer with the
    alpha=0.5 mirror arbiter == the reference's .single/.sing2/.best; the grid never leaves the device."""
    gd = Golden(name)
    st = build_store(eng, gd.problem(oracle))
    pl = st.freeze()
    e = eng.Engine(len(gd.sample_ids), gd.alphas, gd.doublet_prior)
    e.set_genotypes(gd.g); e.set_pileup(pl)
    e.run_singlet(); e.run_doublet()
    llks, llk0s = e.get_singlet()
    grid, l00, summ = e.get_doublet(want_grid=True)
    sing = e.get_sing()
    e.close()
    assert np.array_equal(sing, grid[:, :, 0, 0])
    fa = eng.FinalArgs(st.barcodes(), gd.sample_ids, gd.alphas, gd.doublet_prior, pl.rd_totl, pl.rd_pass, pl.rd_uniq,
                       pl.n_snp_per_cell, gd.min_total, gd.min_uniq, gd.min_snp, False)
    eng.write_single(fa, llks, llk0s, str(tmp_path / "o.single"))
    eng.write_doublet_summary(fa, sing, l00, summ, str(tmp_path / "o"), tie_pileup=pl, tie_g=gd.g)
    for suf in ("single", "sing2", "best"):
        got = (tmp_path / f"o.{suf}").read_text().splitlines()
        want = gd.files[suf].decode().splitlines()
        assert len(got) == len(want)
        for a, b in zip(got, want):
            fa_, fb_ = a.split("\t"), b.split("\t")
            for x, y in zip(fa_, fb_):
                try:
                    fx, fy = float(x), float(y)
                    assert abs(fx - fy) <= 1e-3 * max(1e-3, abs(fy)) + 1.01e-4
                except ValueError:
                    assert x == y, (suf, a, b)


@pytest.mark.parametrize("V,B,S,delta,missing", [(8, 40, 600, 0.3, 0.0), (16, 20, 500, 0.3, 0.1), (32, 12, 400, 0.5, 0.05), (64, 5, 300, 0.3, 0.0), (3, 30, 200, 1.0, 0.2),
                                                 (100, 4, 200, 0.3, 0.05),     # wide panels: j-slabs (class: 3 slabs; general A=2: 3 slabs)
                                                 (128, 3, 150, 0.4, 0.0),      # 4 x 32 rows, the general kernel's LDS limit
                                                 (200, 2, 120, 0.4, 0.1)])     # class K2 in 11 slabs vs the generic slab kernel
@pytest.mark.parametrize("alphas", [(0.0, 0.5), (0.0, 0.25, 0.5), (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)])
def test_genotype_class_kernel_is_bit_identical_to_the_general_one(eng, oracle, V, B, S, delta, missing, alphas):
    """--field GT gives <= 4 distinct probability rows per SNP; the class kernel evaluates log() once per distinct
    (row_j, row_k) and must reproduce the general kernel BIT FOR BIT (same operands, same operations, same add order)."""
    import os
    from demuxlet_amd import synth
    rng = np.random.default_rng(4242 + V)
    raw = synth.make_raw_genotypes(rng, S, V, missing_rate=missing)
    g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    sp = synth.make_pileup(rng, np.where(raw.alleles < 0, 0, raw.alleles), B, delta, 1.5, dense_layout=(delta >= 1.0))
    pl = host_pileup(eng, sp)
    os.environ.pop("DMX_NO_CLASSES", None)
    a = run_engine(eng, pl, g, alphas, 0.5)
    os.environ["DMX_NO_CLASSES"] = "1"
    try:
        b = run_engine(eng, pl, g, alphas, 0.5)
    finally:
        os.environ.pop("DMX_NO_CLASSES", None)
    assert np.array_equal(a["llks"], b["llks"]) and np.array_equal(a["llk0s"], b["llk0s"])      # K1 over classes
    assert np.array_equal(a["grid"], b["grid"]) and np.array_equal(a["l00"], b["l00"])            # K2 over classes
    assert np.array_equal(a["summ"], b["summ"])
    ref = oracle_from_pileup(oracle, sp, g, alphas, 0.5)
    assert np.abs(a["grid"] - ref.llksAB).max() < TOL and np.abs(a["llks"] - ref.llks).max() < TOL


@pytest.mark.parametrize("V,missing,dense,err", [(8, 0.0, True, 0.01), (8, 0.15, True, 0.01), (3, 0.5, False, 0.01), (16, 0.05, False, 0.1),
                                                 (19, 0.3, True, 0.001), (5, 1.0, False, 0.01), (8, 0.1, True, 0.0)])
def test_canonical_gt_classes_are_bit_identical_to_the_plain_class_form(eng, oracle, V, missing, dense, err):
    """Round 4: called genotypes of a --field GT matrix share three SNP-independent rows; the classes are relabelled to them
    (k_canon_apply) and K1 reads log(GL . row) of those three from a table (k_singlet_cls<.., CAN>).  Same expression, same log:
    every output must equal the plain class form's (DMX_NO_CANON=1) bit for bit — on pairs of 0..6 reads with base qualities over
    the whole 0..127 range (the tables cover up to three reads of quality < 48 / two < 64; the rest is evaluated in the kernel),
    with and without missing genotypes (the SNP's own fourth row), through K1, K2 and K3."""
    import os
    from demuxlet_amd import synth
    rng = np.random.default_rng(7100 + V + int(100 * missing))
    S, B = 400, 24
    raw = synth.make_raw_genotypes(rng, S, V, missing_rate=missing)
    g = np.stack([eng.geno_from_gt(raw.alleles[s], err) for s in range(S)])
    if dense:
        npair = np.full(B, S); pair_snp = None
    else:
        cov = rng.random((B, S)) < 0.3
        npair = cov.sum(axis=1)
        pair_snp = np.concatenate([np.nonzero(cov[c])[0] for c in range(B)]).astype(np.int32)
    P = int(npair.sum())
    nrd = rng.choice(np.arange(7), size=P, p=[0.05, 0.45, 0.2, 0.15, 0.05, 0.05, 0.05]).astype(np.uint8)
    nr = int(nrd.sum())
    bq = np.where(rng.random(nr) < 0.8, rng.integers(2, 45, size=nr), rng.integers(0, 128, size=nr)).astype(np.uint8)
    reads = bq | (rng.integers(0, 2, size=nr).astype(np.uint8) << 7)
    cpo = np.concatenate([[0], np.cumsum(npair)]).astype(np.int64)
    cro = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(B), npair), weights=nrd, minlength=B))]).astype(np.int64)
    z = np.zeros(B, dtype=np.int32)
    pl = eng.HostPileup(B, S, cpo, cro, pair_snp, nrd, reads, z, z, z)
    os.environ.pop("DMX_NO_CANON", None)
    a = run_engine(eng, pl, g, (0.0, 0.5), 0.5)
    os.environ["DMX_NO_CANON"] = "1"
    try:
        b = run_engine(eng, pl, g, (0.0, 0.5), 0.5)
    finally:
        os.environ.pop("DMX_NO_CANON", None)
    for f in ("llks", "llk0s", "grid", "l00", "summ"):
        assert np.array_equal(a[f], b[f]), f

    class SP: pass
    sp = SP(); sp.reads = reads; sp.pair_snp = pair_snp; sp.n_snps = S; sp.n_cells = B; sp.pair_nrd = nrd
    sp.cell_pair_off = cpo; sp.rd_totl = sp.rd_pass = sp.rd_uniq = z
    ref = oracle_from_pileup(oracle, sp, g, (0.0, 0.5), 0.5)
    d = max(np.abs(a["llks"] - ref.llks).max(), np.abs(a["llk0s"] - ref.llk0s).max(), np.abs(a["grid"] - ref.llksAB).max())
    assert d < TOL


def test_canonical_gt_classes_fall_back_on_matrices_of_another_shape(eng, oracle):
    """A matrix whose SNPs carry two different non-canonical rows (two genotype-error rates mixed) keeps k_build_classes' labels and the
    plain class kernels; a phred table change rebuilds the canonical-class log table."""
    import os
    from demuxlet_amd import synth
    rng = np.random.default_rng(7177)
    S, V, B = 300, 6, 20
    raw = synth.make_raw_genotypes(rng, S, V, missing_rate=0.1)
    g1 = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    g2 = np.stack([eng.geno_from_gt(raw.alleles[s], 0.05) for s in range(S)])
    g = g1.copy(); g[:, ::2] = g2[:, ::2]                      # every other sample with another error rate: up to 6 rows per SNP -> no classes at all or two "others"
    g3 = g1.copy(); g3[:, 0] = g2[:, 0]                        # one odd sample: <= 4 rows on many SNPs, two non-canonical ones wherever it sits beside a missing genotype
    sp = synth.make_pileup(rng, np.where(raw.alleles < 0, 0, raw.alleles), B, 0.4, 1.5)
    pl = host_pileup(eng, sp)
    for gm in (g, g3):
        os.environ.pop("DMX_NO_CLASSES", None)
        a = run_engine(eng, pl, gm, (0.0, 0.5), 0.5)
        os.environ["DMX_NO_CLASSES"] = "1"
        try:
            b = run_engine(eng, pl, gm, (0.0, 0.5), 0.5)
        finally:
            os.environ.pop("DMX_NO_CLASSES", None)
        for f in ("llks", "llk0s", "grid", "l00", "summ"):
            assert np.array_equal(a[f], b[f]), f
    # new phred tables: the canonical-class log table follows them
    e = eng.Engine(V, (0.0, 0.5), 0.5)
    e.set_genotypes(g1); e.set_pileup(pl)
    e.run_singlet(); first = e.get_singlet()
    mat, errt = eng.phred_tables()
    errt2 = errt.copy(); errt2[20:] *= 0.5
    e.set_phred_tables(1.0 - errt2, errt2)
    e.run_singlet(); second = e.get_singlet()
    e.close()
    os.environ["DMX_NO_CANON"] = "1"
    try:
        e = eng.Engine(V, (0.0, 0.5), 0.5)
        e.set_genotypes(g1); e.set_pileup(pl)
        e.set_phred_tables(1.0 - errt2, errt2)
        e.run_singlet(); want = e.get_singlet()
        e.close()
    finally:
        os.environ.pop("DMX_NO_CANON", None)
    assert not np.array_equal(first[0], second[0])
    assert np.array_equal(second[0], want[0]) and np.array_equal(second[1], want[1])


@pytest.mark.parametrize("V,field,dense", [(8, "GT", True), (32, "GP", True), (16, "PL", False), (40, "GT", False)])
def test_certify_seed_tables_leave_every_record_unchanged(eng, V, field, dense):
    """Round 4: k_certify takes the state after a pair's first one or two reads from a device-built table (k_build_certify_seeds) instead of
    running the read loop from the start.  Same operations on the same operands: every per-barcode record (certificates, bracket values,
    event words, flags) must equal the table-free walk's (DMX_CERTIFY_NO_SEEDS=1) bit for bit — pairs of 0..6 reads (deep ones: the slow
    division), base qualities over the whole range (>= 64: outside the two-read table)."""
    import os
    from demuxlet_amd import synth
    rng = np.random.default_rng(8300 + V)
    S, B = 500, 40
    raw = synth.make_raw_genotypes(rng, S, V, missing_rate=0.05 if field == "GT" else 0.0)
    if field == "GT":
        g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    elif field == "GP":
        g = np.stack([eng.geno_from_gp(x, 0.01) for x in synth.raw_gp_from_alleles(rng, np.where(raw.alleles < 0, 0, raw.alleles))])
    else:
        g = np.stack([eng.geno_from_pl(x) for x in synth.raw_pl_from_alleles(rng, np.where(raw.alleles < 0, 0, raw.alleles))])
    if dense:
        npair = np.full(B, S); pair_snp = None
    else:
        cov = rng.random((B, S)) < 0.3
        npair = cov.sum(axis=1)
        pair_snp = np.concatenate([np.nonzero(cov[c])[0] for c in range(B)]).astype(np.int32)
    P = int(npair.sum())
    nrd = rng.choice(np.arange(7), size=P, p=[0.05, 0.5, 0.25, 0.1, 0.04, 0.03, 0.03]).astype(np.uint8)
    nrd[rng.random(P) < 0.002] = 20                                       # beyond kSafeReads: no seed, the plain division
    nr = int(nrd.sum())
    bq = np.where(rng.random(nr) < 0.85, rng.integers(2, 45, size=nr), rng.integers(0, 128, size=nr)).astype(np.uint8)
    reads = bq | (rng.integers(0, 2, size=nr).astype(np.uint8) << 7)
    cpo = np.concatenate([[0], np.cumsum(npair)]).astype(np.int64)
    cro = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(B), npair), weights=nrd, minlength=B))]).astype(np.int64)
    z = np.zeros(B, dtype=np.int32)
    pl = eng.HostPileup(B, S, cpo, cro, pair_snp, nrd, reads, z, z, z)
    os.environ.pop("DMX_CERTIFY_NO_SEEDS", None)
    os.environ.pop("DMX_CERTIFY_NO_FINALS", None)
    os.environ["DMX_FINALS_ANY_DEPTH"] = "1"          # (the launch rule keeps the table from pileups this small or this deep: lifted here)
    a = run_engine(eng, pl, g, (0.0, 0.5), 0.5)       # round 6: final values of 0..3-read pairs from k_build_certify_finals' table, seeds for the deeper ones
    os.environ.pop("DMX_FINALS_ANY_DEPTH", None)
    os.environ["DMX_CERTIFY_NO_SEEDS"] = "1"
    try:
        b = run_engine(eng, pl, g, (0.0, 0.5), 0.5)   # no table at all
    finally:
        os.environ.pop("DMX_CERTIFY_NO_SEEDS", None)
    os.environ["DMX_CERTIFY_NO_FINALS"] = "1"
    try:
        c = run_engine(eng, pl, g, (0.0, 0.5), 0.5)   # seeds only (rounds 4-5)
    finally:
        os.environ.pop("DMX_CERTIFY_NO_FINALS", None)
    from demuxlet_amd import capi
    assert ((a["summ"]["flags"] & (capi.DMX_CELL_ORDER_CERTIFIED | capi.DMX_CELL_ORDER_RESOLVABLE)) != 0).sum() > B // 4
    assert a["summ"].tobytes() == b["summ"].tobytes()
    assert c["summ"].tobytes() == b["summ"].tobytes()


def test_all_base_qualities_and_depths(eng, oracle):
    """Base qualities over the whole ABI range 0..127 (the first-read tables cover < 64, the rest takes the generic loop,
    q <= 1 has the 0.75 error floor of PhredHelper.cpp:30) and pair depths 0..6, dense and sparse layouts."""
    rng = np.random.default_rng(99)
    for dense in (False, True):
        S, V, B = 200, 5, 30
        g = rng.dirichlet([1, 1, 1], size=(S, V)).astype(np.float32)
        if dense:
            npair = np.full(B, S)
            pair_snp = None
        else:
            cov = rng.random((B, S)) < 0.3
            npair = cov.sum(axis=1)
            pair_snp = np.concatenate([np.nonzero(cov[c])[0] for c in range(B)]).astype(np.int32)
        P = int(npair.sum())
        nrd = rng.integers(0, 7, size=P).astype(np.uint8)
        reads = (rng.integers(0, 128, size=int(nrd.sum())).astype(np.uint8) | (rng.integers(0, 2, size=int(nrd.sum())).astype(np.uint8) << 7))
        cpo = np.concatenate([[0], np.cumsum(npair)]).astype(np.int64)
        pair_cell = np.repeat(np.arange(B), npair)
        cro = np.concatenate([[0], np.cumsum(np.bincount(pair_cell, weights=nrd, minlength=B))]).astype(np.int64)
        z = np.zeros(B, dtype=np.int32)
        pl = eng.HostPileup(B, S, cpo, cro, pair_snp, nrd, reads, z, z, z)
        out = run_engine(eng, pl, g, (0.0, 0.5), 0.5)

        class SP: pass
        sp = SP(); sp.reads = reads; sp.pair_snp = pair_snp; sp.n_snps = S; sp.n_cells = B; sp.pair_nrd = nrd
        sp.cell_pair_off = cpo; sp.rd_totl = sp.rd_pass = sp.rd_uniq = z
        ref = oracle_from_pileup(oracle, sp, g, (0.0, 0.5), 0.5)
        d = max(np.abs(out["llks"] - ref.llks).max(), np.abs(out["llk0s"] - ref.llk0s).max(), np.abs(out["grid"] - ref.llksAB).max())
        print(f"dense={dense}: max|d| = {d:.2e}")
        assert d < TOL


@pytest.mark.parametrize("name", ["gt_v4_a2_pair", "gp_v8_a2_minsnp", "pl_v32_a3", "gt_v64_a2"])
def test_without_the_arbiter_only_the_order_inside_a_doublet_can_differ(eng, oracle, name, tmp_path):
    """arbiter=False: every number comes from the GPU.  The SNG/DBL/AMB call, the best singlets and the UNORDERED best
    doublet pair still equal the reference's; only which of the two samples of an alpha=0.5 doublet is printed first may
    differ (the reference decides that by its own 1e-14 rounding noise)."""
    gd = Golden(name)
    st = build_store(eng, gd.problem(oracle))
    eng.demuxlet_run(st, gd.g, gd.sample_ids, gd.alphas, str(tmp_path / "o"), gd.doublet_prior, gd.min_total, gd.min_uniq,
                     gd.min_snp, gd.write_pair, arbiter=False)
    got = [r.split("\t") for r in (tmp_path / "o.best").read_text().splitlines()[1:]]
    want = [r.split("\t") for r in gd.files["best"].decode().splitlines()[1:]]
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a[0] == b[0] and a[5].split("-")[0] == b[5].split("-")[0]          # barcode, SNG / DBL / AMB
        assert (a[6], a[8]) == (b[6], b[8])                                          # SNG.1ST, SNG.2ND
        assert {a[11], a[12]} == {b[11], b[12]} and a[13] == b[13]                   # unordered DBL pair, ALPHA
        assert abs(float(a[14]) - float(b[14])) < 1.01e-4                            # LLK12


@pytest.mark.parametrize("V,field", [(70, "GP"), (100, "GP"), (128, "PL"), (129, "GP"), (150, "GP"), (200, "PL"), (256, "GP"), (383, "PL"), (384, "GP"),
                                     (385, "GP"), (500, "GP"), (721, "GP"), (1024, "PL"), (1025, "GP")])
def test_wide_panels_against_oracle(eng, oracle, V, field):
    """Panels wider than one workgroup's 64 rows (pooled designs with 70-150 donors), soft genotype fields (no classes):
    the A = 2 kernel in j-slabs up to V = 1024 (tiles of 32, 16 or 8 covered pairs as the staged genotype rows grow, up to 160 KB of a
    CU's LDS), the generic kernel in accumulator slabs beyond."""
    from demuxlet_amd import synth
    rng = np.random.default_rng(900 + V)
    S, B = 150, 3
    raw = synth.make_raw_genotypes(rng, S, V)
    if field == "GP":
        gp = synth.raw_gp_from_alleles(rng, raw.alleles)
        g = np.stack([eng.geno_from_gp(gp[s], 0.01) for s in range(S)])
    else:
        plv = synth.raw_pl_from_alleles(rng, raw.alleles)
        g = np.stack([eng.geno_from_pl(plv[s]) for s in range(S)])
    sp = synth.make_pileup(rng, raw.alleles, B, 0.4, 1.5, dense_layout=False, doublet_rate=0.3)
    ref = oracle_from_pileup(oracle, sp, g, (0.0, 0.5), 0.5)
    out = run_engine(eng, host_pileup(eng, sp), g, (0.0, 0.5), 0.5)
    d = [np.abs(out["llks"] - ref.llks).max(), np.abs(out["llk0s"] - ref.llk0s).max(), np.abs(out["grid"] - ref.llksAB).max(),
         np.abs(out["l00"] - ref.llks00).max()]
    print(f"V={V} {field}: max|d| = " + " ".join(f"{x:.2e}" for x in d))
    assert max(d) < TOL


@pytest.mark.parametrize("V,alphas,field,B,S", [
    (5, (0.0, 0.25, 0.5), "GT", 20, 400),                       # AP = 4, one wavefront per cell, one phase-1 pass of 2
    (16, (0.0, 0.1, 0.3, 0.5), "GP", 12, 300),                  # AP = 4, four cells per workgroup
    (12, (0.0, 0.1, 0.2, 0.3, 0.4, 0.5), "PL", 10, 300),        # AP = 8 (two padding alphas), four phase-1 passes
    (32, (0.0, 0.2, 0.5), "GP", 6, 300),                        # 256 threads per cell
    (64, (0.0, 0.1, 0.2, 0.3, 0.5), "GP", 4, 200),              # AP = 8, j-slabs
    (100, (0.0, 0.25, 0.5), "GP", 3, 150),                      # AP = 4, NK = 8, j-slabs
    (128, (0.0, 0.1, 0.2, 0.3, 0.4, 0.45, 0.48, 0.5), "GT", 2, 120),   # A = 8 exactly, 72 KB of LDS per workgroup
    (200, (0.0, 0.25, 0.5), "GP", 2, 100),                      # soft fields beyond 128 samples: the same kernel with up to 160 KB of LDS
    (368, (0.0, 0.1, 0.3, 0.5), "PL", 2, 80),                   # AP = 4, the widest panel of k_doublet_an<256,8,4>
    (344, (0.0, 0.1, 0.2, 0.3, 0.5), "GP", 2, 80),              # AP = 8, the widest panel of k_doublet_an<256,4,8>
    (345, (0.0, 0.1, 0.2, 0.3, 0.5), "GP", 2, 60),              # one more sample: the generic kernel
])
def test_longer_alpha_grids_against_oracle(eng, oracle, V, alphas, field, B, S):
    """Alpha grids of 3..8 entries run k_doublet_an (the A = 2 kernel's structure with the alphas padded to 4 or 8 per
    pair; the max across ALL alphas of a pair after every read, :626-639, is a butterfly over those lanes)."""
    from demuxlet_amd import synth
    rng = np.random.default_rng(1300 + V + len(alphas))
    raw = synth.make_raw_genotypes(rng, S, V)
    if field == "GT":
        g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    elif field == "GP":
        gp = synth.raw_gp_from_alleles(rng, raw.alleles)
        g = np.stack([eng.geno_from_gp(gp[s], 0.01) for s in range(S)])
    else:
        plv = synth.raw_pl_from_alleles(rng, raw.alleles)
        g = np.stack([eng.geno_from_pl(plv[s]) for s in range(S)])
    sp = synth.make_pileup(rng, raw.alleles, B, 0.4, 2.5, dense_layout=False, doublet_rate=0.3)
    ref = oracle_from_pileup(oracle, sp, g, alphas, 0.5)
    out = run_engine(eng, host_pileup(eng, sp), g, alphas, 0.5)
    d = [np.abs(out["llks"] - ref.llks).max(), np.abs(out["llk0s"] - ref.llk0s).max(), np.abs(out["grid"] - ref.llksAB).max(),
         np.abs(out["l00"] - ref.llks00).max()]
    print(f"V={V} A={len(alphas)} {field}: max|d| = " + " ".join(f"{x:.2e}" for x in d))
    assert max(d) < TOL
    # K3 on the device grid: the reference's scans
    from golden_util import summary_from_grid as ref_summary
    for c in range(B):
        if sp.cell_pair_off[c + 1] == sp.cell_pair_off[c]:
            continue
        want = ref_summary(out["grid"][c], out["l00"][c], alphas, 0.5, int(out["summ"][c]["n_pairs"]), out["summ"].dtype)
        for f in ("i_sing1", "i_sing2", "j_best", "k_best", "n_best"):
            assert out["summ"][c][f] == want[f], (c, f)


@pytest.mark.parametrize("V,B,S,delta,field", [(2, 30, 300, 0.5, "GP"), (3, 30, 300, 0.5, "PL"), (5, 30, 300, 0.5, "GP"), (8, 30, 800, 0.3, "GP"),
                                               (12, 20, 500, 0.4, "PL"), (16, 20, 600, 1.0, "PL"), (17, 12, 300, 0.4, "GP"), (21, 12, 300, 0.4, "GP"),
                                               (26, 12, 300, 0.4, "PL"), (29, 12, 300, 0.4, "GP"), (32, 10, 500, 0.3, "GP"), (33, 6, 300, 0.3, "GP"),
                                               (48, 6, 300, 0.3, "PL"), (57, 4, 300, 0.3, "GP"), (64, 4, 300, 0.3, "GP"), (100, 3, 200, 0.3, "GP"),
                                               # 64 < V <= 512: the same entry set in slabs; beyond 512 soft fields take the STRICT kernel in both modes
                                               (65, 3, 200, 0.3, "PL"), (96, 3, 200, 0.3, "GP"), (97, 2, 150, 0.4, "GP"), (128, 3, 200, 0.3, "GP"),
                                               (129, 2, 120, 0.3, "GP"), (160, 2, 120, 0.3, "PL"), (192, 2, 100, 0.4, "GP"), (193, 2, 100, 0.4, "GP"),
                                               (255, 2, 80, 0.4, "PL"), (256, 2, 100, 1.0, "GP"), (257, 2, 60, 0.4, "GP"),
                                               (300, 2, 70, 0.4, "PL"), (384, 2, 64, 1.0, "GP"), (385, 2, 60, 0.4, "GP"), (512, 2, 60, 0.4, "GP"), (513, 2, 50, 0.4, "GP"),
                                               # GT inputs: the genotype-class form of the same entry set (k_doublet_clsym)
                                               (2, 30, 300, 0.5, "GT"), (4, 30, 300, 0.5, "GT"), (7, 30, 300, 0.5, "GT"), (8, 30, 800, 0.3, "GT"),
                                               (13, 20, 500, 0.4, "GT"), (16, 20, 600, 1.0, "GT"), (24, 12, 300, 0.4, "GT"), (31, 12, 300, 0.4, "GT"),
                                               (32, 10, 500, 0.3, "GT"), (33, 6, 300, 0.3, "GT"), (48, 6, 300, 0.3, "GT"), (63, 4, 300, 0.3, "GT"),
                                               (64, 4, 300, 1.0, "GT"), (100, 3, 200, 0.3, "GT")])
def test_fast_mode_stays_within_tolerance(eng, oracle, V, B, S, delta, field):
    """DMX_MODE_FAST (opt-in): the doublet term is g_j . (pG[n] g_k) with fused multiply-adds instead of the reference's nine-term
    sum; the accumulation order is unchanged.  Every log-likelihood must stay within the 1e-9 of the north star (measured:
    ~1e-13 at these depths), the singlet outputs are untouched (bit-equal to STRICT)."""
    from demuxlet_amd import synth, capi
    rng = np.random.default_rng(5150 + V)
    raw = synth.make_raw_genotypes(rng, S, V)
    if field == "GP":
        gp = synth.raw_gp_from_alleles(rng, raw.alleles)
        g = np.stack([eng.geno_from_gp(gp[s], 0.01) for s in range(S)])
    elif field == "GT":
        g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    else:
        plv = synth.raw_pl_from_alleles(rng, raw.alleles)
        g = np.stack([eng.geno_from_pl(plv[s]) for s in range(S)])
    sp = synth.make_pileup(rng, raw.alleles, B, delta, 1.5, dense_layout=(delta >= 1.0), doublet_rate=0.3)
    ref = oracle_from_pileup(oracle, sp, g, (0.0, 0.5), 0.5)
    strict = run_engine(eng, host_pileup(eng, sp), g, (0.0, 0.5), 0.5)
    e = eng.Engine(V, (0.0, 0.5), 0.5, mode=capi.DMX_MODE_FAST)
    e.set_genotypes(g); e.set_pileup(host_pileup(eng, sp))
    e.run_singlet(); e.run_doublet()
    llks, llk0s = e.get_singlet()
    grid, l00, summ = e.get_doublet()
    e.close()
    assert np.array_equal(llks, strict["llks"]) and np.array_equal(llk0s, strict["llk0s"]) and np.array_equal(l00, strict["l00"])
    from golden_util import printed_mask
    m = printed_mask(V, 2)[None]                            # every entry demuxlet prints or decides on
    d_ref, d_strict = np.abs(grid - ref.llksAB)[np.broadcast_to(m, grid.shape)].max(), np.abs(grid - strict["grid"])[np.broadcast_to(m, grid.shape)].max()
    print(f"V={V} {field}: FAST vs reference {d_ref:.2e}, FAST vs STRICT {d_strict:.2e} (printed entries)")
    assert d_ref < TOL and d_strict < 1e-10
    if not (field == "GT" and V > 64) and V <= 512:        # wide GT panels keep the (bit-identical) STRICT class kernel, V > 512 the STRICT soft-field one
        assert not np.array_equal(grid, strict["grid"])    # it IS a different operation sequence: keep the two modes honest
    if V <= 64 or (V <= 512 and field != "GT"):
        # alpha grid {0, 0.5}: one evaluation per unordered pair, mirrored; the never-printed [j][k != 0][0] hold [j][0][0]
        assert np.array_equal(grid[:, :, :, 1], grid[:, :, :, 1].transpose(0, 2, 1))
        assert np.array_equal(grid[:, :, :, 0], np.broadcast_to(grid[:, :, 0:1, 0], grid[:, :, :, 0].shape))
    # the per-cell records (K3 over the FAST grid) lead to the reference's calls: same singlets, same doublet pair and alpha
    from golden_util import summary_from_grid as ref_summary
    for c in range(B):
        if sp.cell_pair_off[c + 1] == sp.cell_pair_off[c]:
            continue
        want = ref_summary(ref.llksAB[c], ref.llks00[c], (0.0, 0.5), 0.5, int(summ[c]["n_pairs"]), summ.dtype)
        assert (summ[c]["i_sing1"], summ[c]["i_sing2"], summ[c]["n_best"]) == (want["i_sing1"], want["i_sing2"], want["n_best"]), c
        assert {int(summ[c]["j_best"]), int(summ[c]["k_best"])} == {int(want["j_best"]), int(want["k_best"])}, c
        for f in ("sing_llk1", "sing_llk2", "llk12", "llk00_0", "llk00_best"):
            assert abs(summ[c][f] - want[f]) < TOL, (c, f)
        swap = int(summ[c]["j_best"]) != int(want["j_best"])      # the two samples may come in either order (the arbiter's job)
        for f, fs in (("llk1", "llk2"), ("llk2", "llk1"), ("llk10", "llk20"), ("llk20", "llk10")):
            assert abs(summ[c][f] - want[fs if swap else f]) < TOL, (c, f)


@pytest.mark.parametrize("S,delta", [(1, 1.0), (31, 1.0), (32, 1.0), (33, 1.0), (64, 1.0), (65, 1.0), (97, 1.0), (40, 0.03), (200, 0.16)])
@pytest.mark.parametrize("V", [40, 64])
def test_producer_consumer_class_kernel_at_tile_edges(eng, oracle, V, S, delta, monkeypatch):
    """k_doublet_clsp works in tiles of 32 pairs, double-buffered, its phase 2 requesting up to two pairs ahead: barcodes of 0 (sparse case),
    1, 31, 32, 33, 64, 65, 97 pairs — STRICT bit-identical to the uniform-j kernel of round 3 and to the general kernel, FAST within
    1e-10 of STRICT on the printed entries, both against the oracle."""
    from demuxlet_amd import synth, capi
    from golden_util import printed_mask
    rng = np.random.default_rng(9000 + 131 * V + S)
    B = 13
    raw = synth.make_raw_genotypes(rng, S, V, missing_rate=0.1)
    g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    sp = synth.make_pileup(rng, np.where(raw.alleles < 0, 0, raw.alleles), B, delta, 1.6, dense_layout=(delta >= 1.0), doublet_rate=0.3)
    if delta < 0.1:
        assert (np.diff(sp.cell_pair_off) == 0).any() and (np.diff(sp.cell_pair_off) > 0).any()
    for k in ("DMX_CLS_NO_PROD", "DMX_NO_CLASSES", "DMX_FAST_NO_PROD"):
        monkeypatch.delenv(k, raising=False)
    base = run_engine(eng, host_pileup(eng, sp), g, (0.0, 0.5), 0.5)
    ref = oracle_from_pileup(oracle, sp, g, (0.0, 0.5), 0.5)
    proc = ref.processed.astype(bool)
    assert np.abs(base["grid"][proc] - ref.llksAB[proc]).max() < TOL and np.abs(base["l00"][proc] - ref.llks00[proc]).max() < TOL
    for env in ("DMX_CLS_NO_PROD", "DMX_NO_CLASSES"):
        monkeypatch.setenv(env, "1")
        out = run_engine(eng, host_pileup(eng, sp), g, (0.0, 0.5), 0.5)
        monkeypatch.delenv(env)
        for name in ("grid", "l00", "summ"):
            assert np.array_equal(out[name], base[name]), (env, name)
    e = eng.Engine(V, (0.0, 0.5), 0.5, mode=capi.DMX_MODE_FAST)
    e.set_genotypes(g); e.set_pileup(host_pileup(eng, sp))
    e.run_singlet(); e.run_doublet()
    grid, l00, summ = e.get_doublet()
    e.close()
    m = np.broadcast_to(printed_mask(V, 2)[None], grid.shape)
    assert np.abs(grid - base["grid"])[m].max() < 1e-10 and np.array_equal(l00, base["l00"])
    assert np.array_equal(grid[:, :, 0, 0], base["grid"][:, :, 0, 0])


@pytest.mark.parametrize("V", [33, 48, 64])
def test_fast_mode_class_kernels_of_33_to_64_samples_agree(eng, oracle, V, monkeypatch):
    """GT panels of 33..64 samples in FAST mode run k_doublet_clsp<FAST> (round 4); DMX_FAST_NO_PROD=1 keeps k_doublet_clsym, the
    round-3 kernel.  Both evaluate one orientation per unordered pair with the reference's operations, in different orientations:
    printed entries within 1e-10 of each other and of STRICT, the singlet column and llks00 bit-equal, the same calls."""
    from demuxlet_amd import synth, capi
    from golden_util import printed_mask
    rng = np.random.default_rng(777 + V)
    S, B = 400, 9
    raw = synth.make_raw_genotypes(rng, S, V, missing_rate=0.05)
    g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    sp = synth.make_pileup(rng, np.where(raw.alleles < 0, 0, raw.alleles), B, 0.4, 1.5, dense_layout=False, doublet_rate=0.3)
    strict = run_engine(eng, host_pileup(eng, sp), g, (0.0, 0.5), 0.5)

    def fast():
        e = eng.Engine(V, (0.0, 0.5), 0.5, mode=capi.DMX_MODE_FAST)
        e.set_genotypes(g); e.set_pileup(host_pileup(eng, sp))
        e.run_singlet(); e.run_doublet()
        out = e.get_doublet()
        e.close()
        return out
    monkeypatch.delenv("DMX_FAST_NO_PROD", raising=False)
    grid_a, l00_a, summ_a = fast()
    monkeypatch.setenv("DMX_FAST_NO_PROD", "1")
    grid_b, l00_b, summ_b = fast()
    monkeypatch.delenv("DMX_FAST_NO_PROD")
    m = np.broadcast_to(printed_mask(V, 2)[None], grid_a.shape)
    assert np.abs(grid_a - grid_b)[m].max() < 1e-10 and np.abs(grid_a - strict["grid"])[m].max() < 1e-10
    assert np.array_equal(l00_a, l00_b) and np.array_equal(l00_a, strict["l00"])
    assert np.array_equal(grid_a[:, :, 0, 0], strict["grid"][:, :, 0, 0])            # the singlet column IS the reference's sequence
    assert np.array_equal(grid_a[:, :, :, 1], grid_a[:, :, :, 1].transpose(0, 2, 1))  # mirrored
    for f in ("i_sing1", "i_sing2", "n_best"):
        assert np.array_equal(summ_a[f], summ_b[f]), f
    assert all({int(x["j_best"]), int(x["k_best"])} == {int(y["j_best"]), int(y["k_best"])} for x, y in zip(summ_a, summ_b))


@pytest.mark.parametrize("V,alphas,field,B,S", [
    (5, (0.0, 0.25, 0.5), "GP", 20, 400), (16, (0.0, 0.1, 0.3, 0.5), "GP", 12, 300), (12, (0.0, 0.1, 0.2, 0.3, 0.4, 0.5), "PL", 10, 300),
    (32, (0.0, 0.2, 0.5), "GP", 6, 300), (64, (0.0, 0.1, 0.2, 0.3, 0.5), "GP", 4, 200), (100, (0.0, 0.25, 0.5), "GP", 3, 150),
    (128, (0.0, 0.1, 0.2, 0.3, 0.4, 0.45, 0.48, 0.5), "PL", 2, 120),
    (8, (0.0, 0.3), "GP", 20, 400), (24, (0.0, 0.25), "PL", 8, 300), (40, (0.0, 0.5, 0.25), "GP", 4, 200), (7, (0.0, 0.5, 0.5), "GP", 10, 300),
    (13, (0.0, 0.05, 0.15, 0.25, 0.35, 0.45, 0.5), "GP", 6, 250), (77, (0.0, 0.4), "GP", 3, 150),
    # GT inputs with these grids keep the (bit-exact) class kernels in both modes
    (5, (0.0, 0.25, 0.5), "GT", 20, 400), (48, (0.0, 0.3), "GT", 4, 200)])
def test_fast_mode_other_alpha_grids(eng, oracle, V, alphas, field, B, S):
    """DMX_MODE_FAST on alpha grids other than demuxlet's default {0, 0.5} (`--alpha` is a multi-valued option,
    cmd_cram_demuxlet.cpp:57,78-90): k_doublet_anf evaluates the singlet column and every (j, k) of the alphas n >= 1 in bilinear
    form and fills llksAB[j][k != 0][0] with llksAB[j][0][0].  Every printed entry within 1e-9 of the oracle, the singlet stage
    bit-equal to STRICT, the K3 calls the reference's."""
    from demuxlet_amd import synth, capi
    from golden_util import printed_mask, summary_from_grid as ref_summary
    rng = np.random.default_rng(7300 + V + len(alphas))
    raw = synth.make_raw_genotypes(rng, S, V)
    if field == "GT":
        g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    elif field == "GP":
        g = np.stack([eng.geno_from_gp(x, 0.01) for x in synth.raw_gp_from_alleles(rng, raw.alleles)])
    else:
        g = np.stack([eng.geno_from_pl(x) for x in synth.raw_pl_from_alleles(rng, raw.alleles)])
    sp = synth.make_pileup(rng, raw.alleles, B, 0.4, 2.0, dense_layout=False, doublet_rate=0.3)
    ref = oracle_from_pileup(oracle, sp, g, alphas, 0.5)
    strict = run_engine(eng, host_pileup(eng, sp), g, alphas, 0.5)
    e = eng.Engine(V, alphas, 0.5, mode=capi.DMX_MODE_FAST)
    e.set_genotypes(g); e.set_pileup(host_pileup(eng, sp))
    e.run_singlet(); e.run_doublet()
    llks, llk0s = e.get_singlet()
    grid, l00, summ = e.get_doublet()
    e.close()
    A = len(alphas)
    assert np.array_equal(llks, strict["llks"]) and np.array_equal(llk0s, strict["llk0s"]) and np.array_equal(l00, strict["l00"])
    m = np.broadcast_to(printed_mask(V, A)[None], grid.shape)
    d_ref, d_strict = np.abs(grid - ref.llksAB)[m].max(), np.abs(grid - strict["grid"])[m].max()
    print(f"V={V} A={A} {field}: FAST vs reference {d_ref:.2e}, FAST vs STRICT {d_strict:.2e} (printed entries)")
    assert d_ref < TOL and d_strict < 1e-10
    if field != "GT":
        assert not np.array_equal(grid, strict["grid"])      # a different operation sequence, not the STRICT kernel under another name
        assert np.array_equal(grid[:, :, :, 0], np.broadcast_to(grid[:, :, 0:1, 0], grid[:, :, :, 0].shape))
    for c in range(B):
        if sp.cell_pair_off[c + 1] == sp.cell_pair_off[c]:
            continue
        want = ref_summary(ref.llksAB[c], ref.llks00[c], alphas, 0.5, int(summ[c]["n_pairs"]), summ.dtype)
        assert (summ[c]["i_sing1"], summ[c]["i_sing2"]) == (want["i_sing1"], want["i_sing2"]), c
        # the best doublet: same (unordered where alpha = 0.5) pair and alpha unless the reference's own maximum is a near-tie
        if abs(summ[c]["llk12"] - want["llk12"]) < TOL and not (summ[c]["flags"] & capi.DMX_CELL_NEAR_DOUBLET):
            assert summ[c]["n_best"] == want["n_best"], c
            if alphas[int(want["n_best"])] == 0.5:
                assert {int(summ[c]["j_best"]), int(summ[c]["k_best"])} == {int(want["j_best"]), int(want["k_best"])}, c
            else:
                assert (int(summ[c]["j_best"]), int(summ[c]["k_best"])) == (int(want["j_best"]), int(want["k_best"])), c
        for f in ("sing_llk1", "sing_llk2", "llk12", "llk00_0"):
            assert abs(summ[c][f] - want[f]) < TOL, (c, f)


def test_fast_mode_end_to_end_files(eng, oracle, tmp_path):
    """dmx_demuxlet_run in DMX_MODE_FAST (with the tie arbiter) against the oracle's files on a soft-field 24-sample job: every
    string field — barcodes, ids, the BEST call — identical, printed numbers equal up to their last digit."""
    import os
    from demuxlet_amd import synth, capi
    rng = np.random.default_rng(777)
    V, S, B = 24, 400, 30
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([eng.geno_from_gp(x, 0.01) for x in synth.raw_gp_from_alleles(rng, raw.alleles)])
    sp = synth.make_pileup(rng, raw.alleles, B, 0.3, 1.5, dense_layout=False, doublet_rate=0.4)
    bc, snp, umi, allele, bq, newread = synth.pileup_to_events(rng, sp)
    sm = [f"SM{j:02d}" for j in range(V)]
    params = oracle.Params((0.0, 0.5), 0.5, 0, 0, 0, True)
    oracle.run_problem(oracle.Problem(sm, g, oracle.Events(bc, snp, umi, allele, bq, newread), params), str(tmp_path / "ref"))
    st = eng.Store()
    for _ in range(S):
        st.add_snp()
    for e in range(len(bc)):
        c = st.add_cell(bc[e])
        if newread[e]:
            st.count_read(c)
        if snp[e] >= 0:
            st.add_read(int(snp[e]), c, umi[e], int(allele[e]), int(bq[e]))
    eng.demuxlet_run(st, g, sm, (0.0, 0.5), str(tmp_path / "got"), 0.5, 0, 0, 0, True, arbiter=True, n_gpus=2, mode=capi.DMX_MODE_FAST)
    ndiff = 0
    for suf in ("single", "sing2", "best", "pair"):
        got = (tmp_path / f"got.{suf}").read_text().splitlines()
        want = (tmp_path / f"ref.{suf}").read_text().splitlines()
        assert len(got) == len(want) and len(got) > 1, suf
        for a, b in zip(got, want):
            if a == b:
                continue
            fa, fb = a.split("\t"), b.split("\t")
            assert len(fa) == len(fb)
            for x, y in zip(fa, fb):
                if x != y:
                    assert abs(float(x) - float(y)) <= 1e-3 * max(1e-3, abs(float(y))) + 1.01e-4, (suf, a, b)
                    ndiff += 1
    print(f"FAST end to end: {ndiff} printed numbers differ in the last digit")


@pytest.mark.parametrize("V,field,dense", [(8, "GT", True), (8, "GP", True), (5, "GT", False), (16, "PL", False), (24, "GT", False), (40, "GP", True),
                                           (48, "GT", True), (64, "GT", False), (37, "GT", False),       # 33..64 GT: the uniform-j class kernel
                                           (32, "GP", True), (21, "PL", False), (9, "GP", False), (64, "PL", True)])   # soft fields, 9..64: k_singlet_own
def test_every_launch_geometry_gives_the_same_bits(eng, oracle, V, field, dense, monkeypatch):
    """The launchers pick cells-per-wavefront (1, 2, 4) by barcode count, the narrow or the wide class K1 by panel width, and the
    specialised or the generic K2; the big-count choices are never reached by small tests.  Forcing each of them must not
    change a bit of any output (every accumulator is owned by one lane and adds in SNP order whatever the geometry)."""
    from demuxlet_amd import synth
    rng = np.random.default_rng(31 + V)
    S, B = 700, 37
    raw = synth.make_raw_genotypes(rng, S, V, missing_rate=0.05 if field == "GT" else 0.0)
    al = np.where(raw.alleles < 0, 0, raw.alleles)
    if field == "GT":
        g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    elif field == "GP":
        g = np.stack([eng.geno_from_gp(x, 0.01) for x in synth.raw_gp_from_alleles(rng, al)])
    else:
        g = np.stack([eng.geno_from_pl(x) for x in synth.raw_pl_from_alleles(rng, al)])
    sp = synth.make_pileup(rng, al, B, 1.0 if dense else 0.3, 2.0, dense_layout=dense, doublet_rate=0.3)
    pl = host_pileup(eng, sp)
    for k in ("DMX_K1_CW", "DMX_K1_WIDE_V", "DMX_K2_GENERIC", "DMX_NO_CLASSES", "DMX_NO_K1_CLASSES", "DMX_K1_BLOCK_BYTES", "DMX_K1_NO_BLOCKS",
              "DMX_FORCE_CHECK", "DMX_CLS_NO_UJ", "DMX_CLS_NO_PROD", "DMX_K1_NO_OWN"):
        monkeypatch.delenv(k, raising=False)
    base = run_engine(eng, pl, g, (0.0, 0.5), 0.5)
    ref = oracle_from_pileup(oracle, sp, g, (0.0, 0.5), 0.5)
    assert np.abs(base["grid"] - ref.llksAB).max() < TOL and np.abs(base["llks"] - ref.llks).max() < TOL
    variants = [{"DMX_K1_CW": "1"}, {"DMX_K1_CW": "2"}, {"DMX_K1_CW": "4"}, {"DMX_K1_WIDE_V": "2"}, {"DMX_K1_WIDE_V": "1000"},
                {"DMX_K1_CW": "4", "DMX_NO_K1_CLASSES": "1"}, {"DMX_K1_CW": "2", "DMX_NO_K1_CLASSES": "1"}, {"DMX_K2_GENERIC": "1"},
                {"DMX_NO_CLASSES": "1", "DMX_K1_CW": "4"},
                # sparse general K1 walked in SNP blocks (a launch per block, sums parked in between): 3, 11 and 40 blocks of this panel
                {"DMX_NO_K1_CLASSES": "1", "DMX_K1_BLOCK_BYTES": str(256 * (12 * V + 24))},
                {"DMX_NO_K1_CLASSES": "1", "DMX_K1_BLOCK_BYTES": str(64 * (12 * V + 24)), "DMX_K1_CW": "2"},
                {"DMX_NO_K1_CLASSES": "1", "DMX_K1_BLOCK_BYTES": str(16 * (12 * V + 24)), "DMX_K1_CW": "4"},
                # the general K1 of 9..64 samples is k_singlet_own (lanes own their samples' sums; round 5): against k_singlet (pair lanes, chunked
                # ordered sums), plain, in SNP blocks, and with the argument-class test kept
                {"DMX_NO_K1_CLASSES": "1"}, {"DMX_NO_K1_CLASSES": "1", "DMX_K1_NO_OWN": "1"}, {"DMX_NO_K1_CLASSES": "1", "DMX_FORCE_CHECK": "1"},
                {"DMX_NO_K1_CLASSES": "1", "DMX_K1_NO_OWN": "1", "DMX_K1_BLOCK_BYTES": str(64 * (12 * V + 24))},
                # the per-term argument-class test kept although this panel is provably safe (k_check_geno)
                {"DMX_FORCE_CHECK": "1"}, {"DMX_FORCE_CHECK": "1", "DMX_NO_CLASSES": "1"},
                # the class K2 of 33..64-sample GT panels in its look-up form instead of the uniform-j form (VGPR-relative row selection)
                {"DMX_CLS_NO_UJ": "1"},
                # ... and in the round-3 uniform-j form instead of the producer / consumer kernel (k_doublet_clsp)
                {"DMX_CLS_NO_PROD": "1"}]
    for env in variants:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = run_engine(eng, pl, g, (0.0, 0.5), 0.5)
        for k in env:
            monkeypatch.delenv(k)
        for name in ("llks", "llk0s", "grid", "l00"):
            assert np.array_equal(out[name], base[name]), (env, name)
        assert np.array_equal(out["summ"], base["summ"]), env


def test_cells_without_any_covered_snp(eng, oracle, tmp_path):
    """A BAM where no read overlaps a SNP, and barcode ranges made only of uncovered barcodes: the pileup has zero
    pairs, which must not be read as the dense layout (pair_snp == NULL).  The reference writes .single rows for such cells and
    nothing else (cmd_cram_demuxlet.cpp:592)."""
    from demuxlet_amd import synth
    rng = np.random.default_rng(31)
    V, S = 4, 50
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    sm = [f"S{j}" for j in range(V)]

    def run(covered, n_gpus):
        st = eng.Store()
        for _ in range(S):
            st.add_snp()
        bc, snp, umi, allele, bq, newread = [], [], [], [], [], []
        for i in range(6):
            c = st.add_cell(f"BC{i}-1")
            for r in range(3):
                st.count_read(c)
                bc.append(f"BC{i}-1"); newread.append(1)
                if i in covered:
                    st.add_read(5 + r, c, f"U{r}", r % 2, 30)
                    snp.append(5 + r); umi.append(f"U{r}"); allele.append(r % 2); bq.append(30)
                else:
                    snp.append(-1); umi.append(""); allele.append(0); bq.append(0)
        out = tmp_path / f"o{len(covered)}_{n_gpus}"
        eng.demuxlet_run(st, g, sm, (0.0, 0.5), str(out), n_gpus=n_gpus)
        ev = oracle.Events(bc, np.array(snp, dtype=np.int32), umi, np.array(allele, dtype=np.uint8), np.array(bq, dtype=np.uint8),
                           np.array(newread, dtype=np.uint8))
        ref = tmp_path / f"r{len(covered)}_{n_gpus}"
        oracle.run_problem(oracle.Problem(sm, g, ev, oracle.Params()), str(ref))
        for suf in ("single", "sing2", "best"):
            assert Path(f"{out}.{suf}").read_text() == Path(f"{ref}.{suf}").read_text(), (covered, n_gpus, suf)
        return Path(f"{out}.single").read_text().count("\n"), Path(f"{out}.best").read_text().count("\n")

    from pathlib import Path
    assert run(set(), 1) == (1 + 6 * V, 1)                  # nothing covered at all: .single rows only
    assert run(set(), 3) == (1 + 6 * V, 1)
    assert run({0, 1}, 3) == (1 + 6 * V, 3)                 # ranges 2 and 3 hold only uncovered barcodes
    assert run({5}, 2) == (1 + 6 * V, 2)


def test_engines_on_distinct_devices_when_there_are_several(eng, oracle, tmp_path):
    """dmx_job.n_gpus = min(8, visible devices) on DISTINCT devices (skipped on a 1-GPU box, where the other multi-engine tests
    put every engine on device 0): the reference's four files, byte for byte."""
    import torch
    n = min(8, torch.cuda.device_count())
    if n < 2:
        pytest.skip("one visible device")
    gd = Golden("gt_v24_a2_deep")
    st = build_store(eng, gd.problem(oracle))
    eng.demuxlet_run(st, gd.g, gd.sample_ids, gd.alphas, str(tmp_path / "o"), gd.doublet_prior, gd.min_total, gd.min_uniq, gd.min_snp,
                     gd.write_pair, arbiter=True, n_gpus=n)
    for suf, ref in gd.files.items():
        assert (tmp_path / f"o.{suf}").read_bytes() == ref, suf


@pytest.mark.parametrize("V,field,S,B,mode,a0", [(8, "GT", 1500, 300, "strict", 0.0), (16, "GP", 800, 200, "fast", 0.0), (32, "GT", 600, 120, "fast", 0.0),
                                                 (5, "PL", 3000, 200, "strict", 0.0), (64, "GT", 300, 60, "fast", 0.0),
                                                 (12, "GP", 900, 150, "strict", 0.2)])     # alpha[0] != 0: K3b's nine-value phase 1
def test_tie_order_certificate_agrees_with_the_host_arbiter(eng, oracle, tmp_path, V, field, S, B, mode, a0):
    """K3b (k_certify) decides on the device, for most barcodes, in which order the reference names the two samples of an
    alpha = 0.5 best doublet — by bracketing the reference's two accumulators bit for bit (DESIGN.md "Ties").  The host tie
    arbiter re-evaluates both accumulators with the host's log().  Wherever the device claims a certificate the two must agree on
    the order AND on LLK12's bits: writing .sing2/.best from the records as certified must give the same bytes as writing them
    with every certificate wiped (= the arbiter decides every barcode)."""
    from demuxlet_amd import synth, capi
    alphas = (a0, 0.5)
    rng = np.random.default_rng(900 + V)
    raw = synth.make_raw_genotypes(rng, S, V)
    if field == "GT":
        g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    elif field == "GP":
        g = np.stack([eng.geno_from_gp(x, 0.01) for x in synth.raw_gp_from_alleles(rng, raw.alleles)])
    else:
        g = np.stack([eng.geno_from_pl(x) for x in synth.raw_pl_from_alleles(rng, raw.alleles)])
    sp = synth.make_pileup(rng, raw.alleles, B, 0.5, 1.6, dense_layout=False, doublet_rate=0.5)
    pl = host_pileup(eng, sp)
    e = eng.Engine(V, alphas, 0.5, mode=capi.DMX_MODE_FAST if mode == "fast" else capi.DMX_MODE_STRICT)
    e.set_genotypes(g); e.set_pileup(pl)
    e.run_singlet(); e.run_doublet()
    _, l00, summ = e.get_doublet(want_grid=False)
    sing = e.get_sing()
    e.close()
    covered = summ["n_pairs"] > 0
    cert = (summ["flags"] & capi.DMX_CELL_ORDER_CERTIFIED) != 0
    resv = (summ["flags"] & capi.DMX_CELL_ORDER_RESOLVABLE) != 0
    assert not (cert & resv).any()
    frac = cert[covered].mean()
    print(f"V={V} {field} {mode}: {cert.sum()} of {covered.sum()} covered barcodes carry the order certificate ({100 * frac:.1f} %), "
          f"{resv.sum()} more hang on one host log() per accumulator ({100 * resv[covered].mean():.1f} %)")
    assert frac > 0.5
    fa = eng.FinalArgs([f"BC{i:05d}" for i in range(B)], [f"S{j}" for j in range(V)], alphas, 0.5, sp.rd_totl, sp.rd_pass, sp.rd_uniq,
                       pl.n_snp_per_cell)
    eng.write_doublet_summary(fa, sing, l00, summ, str(tmp_path / "cert"), tie_pileup=pl, tie_g=g)
    wiped = summ.copy()
    wiped["flags"] &= ~np.int32(capi.DMX_CELL_ORDER_CERTIFIED | capi.DMX_CELL_ORDER_RESOLVABLE)
    eng.write_doublet_summary(fa, sing, l00, wiped, str(tmp_path / "host"), tie_pileup=pl, tie_g=g)
    for suf in ("sing2", "best"):
        assert (tmp_path / f"cert.{suf}").read_bytes() == (tmp_path / f"host.{suf}").read_bytes(), suf
    # and both are the oracle's files (the arbiter path is what the golden tests pin)
    ref = oracle_from_pileup(oracle, sp, g, alphas, 0.5)
    from golden_util import summary_from_grid
    n_swapped = 0
    for c in np.flatnonzero(cert):
        want = summary_from_grid(ref.llksAB[c], ref.llks00[c], alphas, 0.5, int(summ[c]["n_pairs"]), summ.dtype)
        assert (int(summ[c]["j_best"]), int(summ[c]["k_best"])) == (int(want["j_best"]), int(want["k_best"])), c
        assert summ[c]["llk12"] == want["llk12"], c               # the reference's bits
        n_swapped += int(summ[c]["j_best"] > summ[c]["k_best"])
    print(f"   {n_swapped} certified barcodes name the doublet in descending sample order, as the reference does")
    # the resolvable ones: the reference's accumulators are among the two candidates each, and the host's libm picks them
    done = summ.copy()
    left = eng.resolve_tie_order(done)
    print(f"   {resv.sum() - left} of {resv.sum()} resolvable barcodes resolved by the host libm")
    for c in np.flatnonzero(resv):
        a, b = sorted((int(summ[c]["j_best"]), int(summ[c]["k_best"])))
        assert ref.llksAB[c][a][b][1] in (summ[c]["llk_ab"], summ[c]["llk_ab_alt"]), c
        assert ref.llksAB[c][b][a][1] in (summ[c]["llk_ba"], summ[c]["llk_ba_alt"]), c
        if done[c]["flags"] & capi.DMX_CELL_ORDER_CERTIFIED:
            want = summary_from_grid(ref.llksAB[c], ref.llks00[c], alphas, 0.5, int(summ[c]["n_pairs"]), summ.dtype)
            assert (int(done[c]["j_best"]), int(done[c]["k_best"])) == (int(want["j_best"]), int(want["k_best"])), c
            assert done[c]["llk12"] == want["llk12"] and done[c]["llk_ab"] == ref.llksAB[c][a][b][1] and done[c]["llk_ba"] == ref.llksAB[c][b][a][1], c
            for f in ("llk1", "llk2", "llk10", "llk20"):
                assert abs(done[c][f] - want[f]) < 1e-9, (c, f)
    assert left <= max(1, resv.sum() // 20)


def test_device_warm_up_on_the_gpu(eng):
    """dmx_device_warm_up: OK for device 0 (any n_gpus: devices wrap around the visible ones), DMX_ERR_ARG for a device that is not there;
    an engine created afterwards works as usual."""
    from demuxlet_amd import capi
    eng.device_warm_up(0, 1)
    eng.device_warm_up(0, 3)
    lib = capi.load()
    assert lib.dmx_device_warm_up(4096, 1) == capi.DMX_ERR_ARG
    e = eng.Engine(3, (0.0, 0.5), 0.5)
    e.close()


@pytest.mark.parametrize("V,field,dense,mode", [(8, "GT", True, "strict"), (12, "GP", False, "strict"), (32, "GP", True, "fast"), (64, "GT", False, "fast"),
                                                  (48, "GT", True, "strict"), (5, "PL", False, "fast")])
def test_run_is_singlet_and_doublet_in_one_call(eng, V, field, dense, mode):
    """dmx_engine_run (K1 beside K2 on a low-priority stream, fork / join on the engine's stream): the same bits as run_singlet followed by
    run_doublet, call after call, also when the two styles alternate on one engine."""
    from demuxlet_amd import synth, capi
    rng = np.random.default_rng(4400 + V)
    S, B = 700, 40
    raw = synth.make_raw_genotypes(rng, S, V)
    if field == "GT":
        g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    elif field == "GP":
        g = np.stack([eng.geno_from_gp(x, 0.01) for x in synth.raw_gp_from_alleles(rng, raw.alleles)])
    else:
        g = np.stack([eng.geno_from_pl(x) for x in synth.raw_pl_from_alleles(rng, raw.alleles)])
    sp = synth.make_pileup(rng, raw.alleles, B, 1.0 if dense else 0.3, 1.5, dense_layout=dense, doublet_rate=0.3)
    e = eng.Engine(V, (0.0, 0.5), 0.5, mode=capi.DMX_MODE_FAST if mode == "fast" else capi.DMX_MODE_STRICT)
    e.set_genotypes(g); e.set_pileup(host_pileup(eng, sp))
    e.run_singlet(); e.run_doublet()
    want = (e.get_singlet(), e.get_doublet())
    for _ in range(3):
        e.run()
        got = (e.get_singlet(), e.get_doublet())
        for a, b in zip(want[0] + want[1], got[0] + got[1]):
            assert np.array_equal(a, b) if a.dtype.names is None else a.tobytes() == b.tobytes()
    e.run_singlet(); e.run_doublet()
    again = (e.get_singlet(), e.get_doublet())
    for a, b in zip(want[0] + want[1], again[0] + again[1]):
        assert a.tobytes() == b.tobytes()
    e.close()


@pytest.mark.parametrize("V,field,dense,mode,sorted_ids", [(8, "GT", True, "strict", True), (12, "GP", False, "strict", False), (33, "GT", False, "fast", False),
                                                           (16, "PL", False, "fast", True), (5, "GT", False, "strict", False),
                                                           (9, "GP", False, "strict", False), (6, "GT", False, "strict", True)])   # V = 9, 6: a three-alpha grid
def test_demuxlet_run_from_a_device_resident_pileup(eng, oracle, tmp_path, monkeypatch, V, field, dense, mode, sorted_ids):
    """dmx_job.pileup with memory = DMX_MEM_DEVICE: the five pileup arrays live in HBM, nothing is sliced or copied on
    the host; ranges of consecutive barcodes are views of the caller's arrays, others are gathered on the device, and the barcodes the tie
    arbiter has to walk get their pieces fetched.  Byte-identical files to the same job from the host pileup — one range and many
    (DMX_RANGE_BYTES), with and without --write-pair — and those are the oracle's."""
    import torch
    from demuxlet_amd import synth, capi
    rng = np.random.default_rng(4100 + V)
    S, B = 500, 300
    alphas = (0.0, 0.25, 0.5) if V in (9, 6) else (0.0, 0.5)       # A = 3: no device certificate, every alpha-0.5 best doublet goes to the arbiter
    raw = synth.make_raw_genotypes(rng, S, V)
    if V == 5:                                     # duplicate samples: near-tie flags, barcodes whose grids AND pileup pieces are fetched
        raw.alleles[:, 1] = raw.alleles[:, 0]; raw.alleles[:, 3] = raw.alleles[:, 2]
    if field == "GT":
        g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    elif field == "GP":
        g = np.stack([eng.geno_from_gp(x, 0.01) for x in synth.raw_gp_from_alleles(rng, raw.alleles)])
    else:
        g = np.stack([eng.geno_from_pl(x) for x in synth.raw_pl_from_alleles(rng, raw.alleles)])
    sp = synth.make_pileup(rng, raw.alleles, B, 1.0 if dense else (0.03 if V == 5 else 0.3), 1.5, dense_layout=dense, doublet_rate=0.4)
    pl = host_pileup(eng, sp)
    bcs = [f"BC{i:05d}-1" for i in range(B)] if sorted_ids else [f"BC{(i * 7919) % 100003:06d}-1" for i in range(B)]
    sms = [f"S{j:02d}" for j in range(V)]
    md = capi.DMX_MODE_FAST if mode == "fast" else capi.DMX_MODE_STRICT
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(pl, k))).to(dev) for k in ("cell_pair_off", "cell_read_off", "pair_nrd", "reads")}
    t_snp = torch.from_numpy(np.ascontiguousarray(pl.pair_snp)).to(dev) if pl.pair_snp is not None else None
    hs = pl.as_struct()                            # (normalises the host arrays; the counters below stay host memory)
    ds = capi.Pileup(B, S, hs.n_pairs, hs.n_reads, t["cell_pair_off"].data_ptr(), t["cell_read_off"].data_ptr(),
                     t_snp.data_ptr() if t_snp is not None else None, t["pair_nrd"].data_ptr(), pl.pair_nrd.dtype.itemsize, capi.DMX_MEM_DEVICE,
                     t["reads"].data_ptr(), pl.rd_totl.ctypes.data, pl.rd_pass.ctypes.data, pl.rd_uniq.ctypes.data)
    ref = oracle_from_pileup_files(oracle, sp, g, alphas, bcs, sms, tmp_path / "orc")
    for tag, rb, wp in (("one", None, False), ("many", "6000", False), ("pair", "30000", True)):
        if rb: monkeypatch.setenv("DMX_RANGE_BYTES", rb)
        else: monkeypatch.delenv("DMX_RANGE_BYTES", raising=False)
        th = eng.demuxlet_run(pl, g, sms, alphas, str(tmp_path / f"h_{tag}"), write_pair=wp, barcodes=bcs, mode=md, timing=True)
        td = eng.demuxlet_run(ds, g, sms, alphas, str(tmp_path / f"d_{tag}"), write_pair=wp, barcodes=bcs, mode=md, timing=True)
        assert td["n_ranges"] == th["n_ranges"] and (rb is None or td["n_ranges"] > 2)
        assert td["n_cells_grid_fetched"] == th["n_cells_grid_fetched"]
        if tag == "one":
            fetched_one = th["n_cells_grid_fetched"]
        for suf in ("single", "sing2", "best") + (("pair",) if wp else ()):
            a, b = (tmp_path / f"d_{tag}.{suf}").read_bytes(), (tmp_path / f"h_{tag}.{suf}").read_bytes()
            assert a == b, (tag, suf)
            if mode == "strict":
                assert a == (tmp_path / f"orc.{suf}").read_bytes(), (tag, suf)
    if V == 5:
        assert fetched_one > 10
    # n_gpus > 1 is refused for a device-resident pileup
    with pytest.raises(Exception, match="one GPU"):
        eng.demuxlet_run(ds, g, sms, alphas, str(tmp_path / "x"), barcodes=bcs, n_gpus=2)


@pytest.mark.parametrize("sorted_ids", [False, True], ids=["gathered", "views"])
def test_demuxlet_run_dense_headline_over_ranges(eng, oracle, tmp_path, monkeypatch, sorted_ids):
    """The case (32, "GP", dense, STRICT) of test_demuxlet_run_from_a_device_resident_pileup at a small shape of its own (that test's 300 barcodes x 500 SNPs
    and its DMX_RANGE_BYTES would make 300 ranges of one barcode each): the ranges of dmx_demuxlet_run on top of k_doublet_a2u<k_doublet_a2u2> — views of the
    caller's device arrays with a non-zero first cell (sorted ids), ranges gathered on the device from non-consecutive cells (unsorted ids), two-byte read
    counts, the K3 records, the certificate and the writers.  Byte-identical files from the device-resident and the host pileup, and those are the oracle's."""
    import torch
    from demuxlet_amd import synth, capi
    from quality_mix import genotypes, mixed_depth_pileup
    V, S, B = 32, 70, 11
    alphas = (0.0, 0.5)
    rng = np.random.default_rng(4132)
    raw = synth.make_raw_genotypes(rng, S, V)
    g = genotypes(eng, rng, raw.alleles, "GP")
    sp = mixed_depth_pileup(rng, raw.alleles, B, 1.0, quals="edges", dense=True, deep=2, doublet_rate=0.4)
    assert sp.pair_snp is None and sp.pair_nrd.dtype == np.uint16
    pl = host_pileup(eng, sp)
    # unsorted: barcode i is the (7 i mod 11)-th in output order, so consecutive output rows are cells 8 apart (mod 11) and no range is a run of consecutive cells
    bcs = [f"BC{i:05d}-1" for i in range(B)] if sorted_ids else [f"BC{(i * 7) % B:05d}-1" for i in range(B)]
    sms = [f"S{j:02d}" for j in range(V)]
    # the engine runs the two-barcode kernel on this pileup (the job itself does not report kernel names)
    monkeypatch.setenv("DMX_EXPERIMENTS", "1")
    e = eng.Engine(V, alphas, 0.5)
    e.set_genotypes(g); e.set_pileup(pl); e.run(); e.sync()
    names = e.kernel_names(); e.close()
    assert names["doublet"] == "k_doublet_a2u<k_doublet_a2u2>", names
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(pl, k))).to(dev) for k in ("cell_pair_off", "cell_read_off", "pair_nrd", "reads")}
    hs = pl.as_struct()
    ds = capi.Pileup(B, S, hs.n_pairs, hs.n_reads, t["cell_pair_off"].data_ptr(), t["cell_read_off"].data_ptr(), None, t["pair_nrd"].data_ptr(),
                     pl.pair_nrd.dtype.itemsize, capi.DMX_MEM_DEVICE, t["reads"].data_ptr(), pl.rd_totl.ctypes.data, pl.rd_pass.ctypes.data,
                     pl.rd_uniq.ctypes.data)
    oracle_from_pileup_files(oracle, sp, g, alphas, bcs, sms, tmp_path / "orc")
    # Ranges (dmx_demuxlet_run): a barcode's grid is 32 x 32 x 2 doubles = 16 384 bytes, and the eleven barcodes are equal work (70 pairs each).
    #   DMX_RANGE_BYTES = 50 000: at most 3 barcodes per range, ceil(11 x 16 384 / 50 000) = 4 ranges, cut where the work passes 11 r / 4 barcodes = after 3, 6
    #     and 9: ranges of 3, 3, 3 and 2 barcodes — the first three are odd (one full workgroup and a lone last barcode), and start at cells 0, 3, 6, 9.
    #   DMX_RANGE_BYTES = 90 000: at most 5 per range, ceil(11 x 16 384 / 90 000) = 3 ranges, cut after 4 and 8: ranges of 4, 4 and 3 — the last one is odd.
    for tag, rb, wp, n_ranges in (("one", None, False, 1), ("many", "50000", False, 4), ("pair", "90000", True, 3)):
        if rb: monkeypatch.setenv("DMX_RANGE_BYTES", rb)
        else: monkeypatch.delenv("DMX_RANGE_BYTES", raising=False)
        th = eng.demuxlet_run(pl, g, sms, alphas, str(tmp_path / f"h_{tag}"), write_pair=wp, barcodes=bcs, timing=True)
        td = eng.demuxlet_run(ds, g, sms, alphas, str(tmp_path / f"d_{tag}"), write_pair=wp, barcodes=bcs, timing=True)
        assert td["n_ranges"] == th["n_ranges"] == n_ranges, (tag, td["n_ranges"], th["n_ranges"])
        assert td["n_cells_grid_fetched"] == th["n_cells_grid_fetched"]
        for suf in ("single", "sing2", "best") + (("pair",) if wp else ()):
            a, b = (tmp_path / f"d_{tag}.{suf}").read_bytes(), (tmp_path / f"h_{tag}.{suf}").read_bytes()
            assert a == b, (tag, suf)
            assert a == (tmp_path / f"orc.{suf}").read_bytes(), (tag, suf)


def oracle_from_pileup_files(oracle, sp, g, alphas, barcodes, sample_ids, prefix):
    al = (sp.reads >> 7).astype(np.uint32)
    words = (al << 24) | ((sp.reads & 0x7F).astype(np.uint32) << 16) | 1
    pair_snp = sp.pair_snp if sp.pair_snp is not None else np.tile(np.arange(sp.n_snps, dtype=np.int32), sp.n_cells)
    csr = oracle.Csr(list(barcodes), sp.cell_pair_off, pair_snp, np.concatenate([[0], np.cumsum(sp.pair_nrd.astype(np.int64))]), words.astype(np.uint32),
                     sp.rd_totl, sp.rd_pass, sp.rd_uniq)
    return oracle.run_csr(csr, list(sample_ids), g, oracle.Params(tuple(alphas), 0.5, 0, 0, 0, True), str(prefix))


def test_experiment_switches_are_fenced(eng, monkeypatch):
    """the DMX_* variables that pick kernel variants are experiment switches, not API.  An engine copies them once, at
    dmx_engine_create, and only when DMX_EXPERIMENTS=1; a stray variable in a user's environment changes nothing, and neither does one set
    after the engine exists.  dmx_engine_kernel_names says which kernels ran (rocprofv3's names)."""
    from demuxlet_amd import synth
    rng = np.random.default_rng(5)
    S, V, B = 300, 8, 16
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    pl = host_pileup(eng, synth.make_pileup(rng, raw.alleles, B, 0.4, 1.5))

    def names(after_create=None):
        e = eng.Engine(V, (0.0, 0.5), 0.5)
        if after_create:
            after_create()
        e.set_genotypes(g); e.set_pileup(pl); e.run(); e.sync()
        n = e.kernel_names(); e.close()
        return n

    monkeypatch.setenv("DMX_EXPERIMENTS", "1")
    monkeypatch.delenv("DMX_NO_CLASSES", raising=False)
    base = names()
    assert base["singlet"].startswith("k_singlet_can<") and base["doublet"].startswith("k_doublet_cls<") and base["certify"].startswith("k_certify<"), base
    assert base["k1_placement"] == 1
    monkeypatch.setenv("DMX_NO_CLASSES", "1")
    forced = names()
    assert forced["singlet"].startswith("k_singlet<") and forced["doublet"].startswith("k_doublet_a2<"), forced       # honoured with the fence open
    monkeypatch.setenv("DMX_EXPERIMENTS", "0")
    assert names() == base                                                                                            # ignored with the fence shut
    monkeypatch.delenv("DMX_EXPERIMENTS")
    assert names() == base
    monkeypatch.setenv("DMX_EXPERIMENTS", "1")
    monkeypatch.delenv("DMX_NO_CLASSES")
    assert names(after_create=lambda: monkeypatch.setenv("DMX_NO_CLASSES", "1")) == base                              # read at create, not per launch
    monkeypatch.delenv("DMX_NO_CLASSES")

    # ... and so are the three variables that change how dmx_demuxlet_run cuts a job: DMX_RANGE_BYTES, DMX_RANGES_PER_GPU,
    # DMX_ONE_ENGINE_PER_GPU.  With the fence shut a stray one cannot change a user's ranges or engines.
    import tempfile
    bcs = [f"BC{i:03d}-1" for i in range(B)]
    sms = [f"S{j}" for j in range(V)]

    def job():
        with tempfile.TemporaryDirectory() as td:
            t = eng.demuxlet_run(pl, g, sms, (0.0, 0.5), td + "/o", barcodes=bcs, timing=True)
        return t["n_ranges"], t["n_engines"]

    for k in ("DMX_RANGE_BYTES", "DMX_RANGES_PER_GPU", "DMX_ONE_ENGINE_PER_GPU"):
        monkeypatch.delenv(k, raising=False)
    assert job() == (1, 1)
    for fence in (None, "0"):
        if fence is None: monkeypatch.delenv("DMX_EXPERIMENTS", raising=False)
        else: monkeypatch.setenv("DMX_EXPERIMENTS", fence)
        monkeypatch.setenv("DMX_RANGE_BYTES", "4096")
        assert job() == (1, 1)
        monkeypatch.delenv("DMX_RANGE_BYTES")
        monkeypatch.setenv("DMX_RANGES_PER_GPU", "4")
        assert job() == (1, 1)
        monkeypatch.delenv("DMX_RANGES_PER_GPU")
    monkeypatch.setenv("DMX_EXPERIMENTS", "1")
    monkeypatch.setenv("DMX_RANGES_PER_GPU", "4")
    assert job() == (4, 2)                                                                                           # four ranges, two alternating engines
    monkeypatch.setenv("DMX_ONE_ENGINE_PER_GPU", "1")
    assert job() == (4, 1)
    monkeypatch.setenv("DMX_EXPERIMENTS", "0")
    assert job() == (1, 1)


def test_fast_mode_keeps_the_lite_log_away_from_very_deep_barcodes(eng, monkeypatch):
    """dmx_log2_lite's worst case is linear in the number of terms (5.7e-15 each), so a pileup whose longest barcode covers more than 130 000 SNPs
    runs the STRICT kernels in FAST mode too (bit-exact, inside FAST's contract).  One barcode of 130 001 covered SNPs on a soft field: the doublet kernel
    is k_doublet_a2, not k_doublet_sym; one SNP fewer: k_doublet_sym."""
    from demuxlet_amd import synth, capi
    rng = np.random.default_rng(8)
    V = 6                                           # (up to four samples a soft field still has <= 4 distinct rows per SNP and runs the class kernels)
    for S, want in ((130001, "k_doublet_a2<"), (130000, "k_doublet_sym<")):
        raw = synth.make_raw_genotypes(rng, S, V)
        g = np.stack([eng.geno_from_gp(x, 0.01) for x in synth.raw_gp_from_alleles(rng, raw.alleles)])
        sp = synth.make_pileup(rng, raw.alleles, 2, 1.0, 1.1, dense_layout=True)
        e = eng.Engine(V, (0.0, 0.5), 0.5, mode=capi.DMX_MODE_FAST)
        e.set_genotypes(g); e.set_pileup(host_pileup(eng, sp)); e.run(); e.sync()
        assert e.kernel_names()["doublet"].startswith(want), (S, e.kernel_names())
        e.close()


@pytest.mark.parametrize("V", [9, 12, 13, 16])
def test_counted_row_wait_equals_waiting_for_everything(eng, monkeypatch, V):
    """the two-barcodes-per-wavefront form of k_doublet_sym (V = 9..16) requests genotype rows two sub-tiles ahead into three LDS buffers and
    waits with a hand-counted s_waitcnt vmcnt(SUB x pieces) instead of vmcnt(0).  Stress: barcodes of very unequal length sharing a wavefront (one of them
    empty), tile counts that leave every partial last sub-tile (1, 2, 3 pairs), sparse SNP ids over a matrix far beyond the L2 (slow, reordered-looking row
    fetches) — the counted form, the vmcnt(0) form (DMX_SYM_WAIT_ALL=1) and the no-DMA form give the same bits, three runs each."""
    from demuxlet_amd import synth, capi
    rng = np.random.default_rng(1300 + V)
    S, B = 60000, 97
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([eng.geno_from_gp(x, 0.01) for x in synth.raw_gp_from_alleles(rng, raw.alleles)])
    sp = synth.make_pileup(rng, raw.alleles, B, 0.02, 1.6, doublet_rate=0.3)
    # unequal lengths: cut every barcode to a chosen number of pairs (0, 1 .. 19 — every residue of the 16-pair tile and the 4-pair sub-tile — and long ones)
    keep = [0, 1, 2, 3, 5, 6, 7, 9, 13, 15, 16, 17, 18, 19, 33, 47, 64, 65] + list(rng.integers(20, 1100, size=B - 18))
    po = sp.cell_pair_off
    sel = np.concatenate([np.arange(po[c], min(po[c + 1], po[c] + keep[c])) for c in range(B)]).astype(np.int64)
    nrd = sp.pair_nrd.astype(np.int64)
    ro = np.concatenate([[0], np.cumsum(nrd)])
    rsel = np.concatenate([np.arange(ro[p], ro[p + 1]) for p in sel]) if len(sel) else np.zeros(0, np.int64)
    npair = np.array([min(po[c + 1] - po[c], keep[c]) for c in range(B)], dtype=np.int64)
    cpo = np.concatenate([[0], np.cumsum(npair)])
    cro = np.concatenate([[0], np.cumsum([nrd[sel[cpo[c]:cpo[c + 1]]].sum() for c in range(B)])]).astype(np.int64)
    pl = eng.HostPileup(B, S, cpo, cro, sp.pair_snp[sel], sp.pair_nrd[sel], sp.reads[rsel], sp.rd_totl, sp.rd_pass, sp.rd_uniq)

    def run(env):
        monkeypatch.setenv("DMX_EXPERIMENTS", "1")
        for k in ("DMX_SYM_WAIT_ALL", "DMX_SYM_NO_DMA"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = eng.Engine(V, (0.0, 0.5), 0.5, mode=capi.DMX_MODE_FAST)
        e.set_genotypes(g); e.set_pileup(pl); e.run(); e.sync()
        assert e.kernel_names()["doublet"].startswith("k_doublet_sym<32, 16, 4,"), e.kernel_names()
        grid, l00, _ = e.get_doublet()
        e.close()
        return grid, l00

    base = run({})
    for env in ({}, {}, {"DMX_SYM_WAIT_ALL": "1"}, {"DMX_SYM_NO_DMA": "1"}, {"DMX_SYM_NO_PIPE": "1"}):
        got = run(env)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), env


def _mixed_depth_problem(eng, V, dense):
    """Soft-field genotypes and a pileup with pairs of 0..6 reads (and a few beyond kSafeReads), base qualities over the whole range, and alternating 64-pair
    blocks without a pair deeper than three reads (tiles that skip the phase-1 read loop) — the inputs of the final-value-table tests."""
    from demuxlet_amd import synth
    rng = np.random.default_rng(9100 + V + (1 if dense else 0))
    S, B = 700, 37
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([eng.geno_from_gp(x, 0.01) for x in synth.raw_gp_from_alleles(rng, raw.alleles)])
    if dense:
        npair = np.full(B, S); pair_snp = None
    else:
        cov = rng.random((B, S)) < 0.3
        npair = cov.sum(axis=1)
        pair_snp = np.concatenate([np.nonzero(cov[c])[0] for c in range(B)]).astype(np.int32)
    P = int(npair.sum())
    nrd = rng.choice(np.arange(7), size=P, p=[0.05, 0.55, 0.25, 0.1, 0.02, 0.02, 0.01]).astype(np.uint8)
    blocks = (np.arange(P) // 64) % 2 == 0
    nrd[blocks & (nrd > 3)] = 1
    nrd[rng.random(P) < 0.001] = 20                                       # beyond kSafeReads
    nr = int(nrd.sum())
    bq = np.where(rng.random(nr) < 0.85, rng.integers(2, 45, size=nr), rng.integers(0, 128, size=nr)).astype(np.uint8)
    reads = bq | (rng.integers(0, 2, size=nr).astype(np.uint8) << 7)
    cpo = np.concatenate([[0], np.cumsum(npair)]).astype(np.int64)
    cro = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(B), npair), weights=nrd, minlength=B))]).astype(np.int64)
    z = np.zeros(B, dtype=np.int32)
    return g, eng.HostPileup(B, S, cpo, cro, pair_snp, nrd, reads, z, z, z)


def _grid_with_env(eng, monkeypatch, g, pl, V, mode, env, kernel_prefix, alphas=(0.0, 0.5)):
    monkeypatch.setenv("DMX_EXPERIMENTS", "1")
    for k in ("DMX_SYM_NO_FINALS", "DMX_A2_NO_FINALS", "DMX_FINALS_ANY_DEPTH", "DMX_A2_SYM", "DMX_A2S_MINW4", "DMX_SYM_NO_SEEDS", "DMX_A2_NO_SEEDS", "DMX_A2_NO_SYMU"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = eng.Engine(V, alphas, 0.5, mode=mode)
    e.set_genotypes(g); e.set_pileup(pl); e.run(); e.sync()
    assert e.kernel_names()["doublet"].startswith(kernel_prefix), e.kernel_names()
    grid, l00, _ = e.get_doublet()
    e.close()
    return grid, l00


@pytest.mark.parametrize("V,dense", [(8, True), (12, False), (16, False), (16, True), (20, True), (32, True), (32, False), (40, False), (64, True), (70, False)])
def test_phase1_final_tables_leave_the_fast_grid_unchanged(eng, monkeypatch, V, dense):
    """Round 6: k_doublet_sym's phase 1 takes the FINISHED values of pairs of up to three tabled reads (no read, one read, two of base quality < 64, three of
    base quality < 48) from k_build_certify_finals' table and runs its read loop only in tiles with a deeper pair.  Same operations on the same operands:
    the grid and llks00 must equal the table-free kernel's (DMX_SYM_NO_FINALS=1) bit for bit — pairs of 0..6 reads and beyond kSafeReads (the plain division),
    base qualities over the whole range, tiles with and without a deep pair, every panel form of the kernel (4 / 2 / 1 barcodes per wavefront, 256-thread
    workgroups, entry slabs).  DMX_FINALS_ANY_DEPTH=1 lifts the launch rule (<= 1.6 reads per pair, >= 1e8 covered pairs) so that these small, deeper pileups exercise the table."""
    from demuxlet_amd import capi
    g, pl = _mixed_depth_problem(eng, V, dense)
    base = _grid_with_env(eng, monkeypatch, g, pl, V, capi.DMX_MODE_FAST, {"DMX_SYM_NO_FINALS": "1", "DMX_SYM_NO_SEEDS": "1"}, "k_doublet_sym<")
    # ... and the pairs that do walk the loop start it from the seed table (the state after their first one or two reads): DMX_SYM_NO_SEEDS=1 is the loop from read 0
    for env in ({"DMX_SYM_NO_FINALS": "1"}, {"DMX_FINALS_ANY_DEPTH": "1"}, {"DMX_FINALS_ANY_DEPTH": "1", "DMX_SYM_NO_SEEDS": "1"}, {}):
        got = _grid_with_env(eng, monkeypatch, g, pl, V, capi.DMX_MODE_FAST, env, "k_doublet_sym<")
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), env
    assert np.isfinite(base[0]).all()


@pytest.mark.parametrize("V,dense", [(5, True), (8, False), (16, True), (24, False), (32, True), (40, False), (130, True)])
def test_phase1_final_tables_leave_the_strict_grid_unchanged(eng, monkeypatch, V, dense):
    """The same table in STRICT's k_doublet_a2 (default grid {0, 0.5} only: the table holds that grid's mixing weights): alpha 0.5's five distinct values and
    alpha 0's three expand to the nine per alpha the read loop computes — entries of equal weight go through identical operations.  Bit for bit against
    DMX_A2_NO_FINALS=1 on every form of the kernel (64-thread cells, 256-thread cells with binary64 rows, j-slabs, the wide-panel tiles); another grid keeps the loop."""
    from demuxlet_amd import capi
    g, pl = _mixed_depth_problem(eng, V, dense)
    base = _grid_with_env(eng, monkeypatch, g, pl, V, capi.DMX_MODE_STRICT, {"DMX_A2_NO_FINALS": "1", "DMX_A2_NO_SEEDS": "1"}, "k_doublet_a2")
    # ... and on that grid the tiles that walk the loop walk it in the five-value form from the seed table (DMX_A2_NO_SEEDS=1: the nine-value loop from read 0)
    for env in ({"DMX_A2_NO_FINALS": "1"}, {"DMX_FINALS_ANY_DEPTH": "1"}, {"DMX_FINALS_ANY_DEPTH": "1", "DMX_A2_NO_SEEDS": "1"}, {}):
        got = _grid_with_env(eng, monkeypatch, g, pl, V, capi.DMX_MODE_STRICT, env, "k_doublet_a2")
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), env
    if V == 16:                                  # a grid the table does not describe: the loop runs, the switch changes nothing
        a = _grid_with_env(eng, monkeypatch, g, pl, V, capi.DMX_MODE_STRICT, {"DMX_FINALS_ANY_DEPTH": "1"}, "k_doublet_a2<", alphas=(0.1, 0.5))
        b = _grid_with_env(eng, monkeypatch, g, pl, V, capi.DMX_MODE_STRICT, {"DMX_A2_NO_FINALS": "1"}, "k_doublet_a2<", alphas=(0.1, 0.5))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("V,B,S,deep", [(8, 37, 700, False), (8, 7, 64, False), (8, 8, 129, False), (5, 100, 333, False), (4, 6, 50, False), (3, 15, 1000, False),
                                        (1, 9, 200, False), (8, 1, 65, False), (7, 64, 4096, False), (8, 30, 1500, True), (6, 10, 257, True)])
def test_producer_consumer_k1_gives_k_singlet_cans_bits(eng, oracle, monkeypatch, V, B, S, deep):
    """Round 6 (an experiment kernel, DMX_K1_CANP=1; not faster than k_singlet_can): k_singlet_canp (dense pileups, canonical GT classes, <= 8
    samples, no fourth genotype row) — seven producer wavefronts put one 32-byte
    record per pair into an LDS ring, one consumer wavefront's 63 lanes own the 7 x 9 chains.  The chains add the doubles k_singlet_can adds, in its order:
    llks and llk0s must be bit-identical (DMX_K1_NO_CANP=1), on barcode counts that are not multiples of 7, SNP counts that are not multiples of 64 (a partial
    last tile), pairs of 0..6 reads and beyond kSafeReads, base qualities beyond
    the tables; and both agree with the oracle."""
    from demuxlet_amd import synth, capi
    rng = np.random.default_rng(7700 + 13 * V + B)
    raw = synth.make_raw_genotypes(rng, S, V, missing_rate=0.0)
    g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    npair = np.full(B, S)                                                 # the dense layout: every barcode covers every SNP (pair index = SNP index)
    P = int(npair.sum())
    nrd = rng.choice(np.arange(7), size=P, p=[0.05, 0.55, 0.25, 0.1, 0.02, 0.02, 0.01]).astype(np.uint8)
    nrd[rng.random(P) < 0.002] = 20
    if deep:                                     # stretches of 3..6 reads per pair: whole tiles on the slow path (reads beyond the tables)
        run_ = (np.arange(P) // 300) % 3 == 1
        nrd[run_] = rng.integers(3, 7, size=int(run_.sum())).astype(np.uint8)
    nr = int(nrd.sum())
    bq = np.where(rng.random(nr) < 0.85, rng.integers(2, 45, size=nr), rng.integers(0, 128, size=nr)).astype(np.uint8)
    reads = bq | (rng.integers(0, 2, size=nr).astype(np.uint8) << 7)
    cpo = np.concatenate([[0], np.cumsum(npair)]).astype(np.int64)
    cro = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(B), npair), weights=nrd, minlength=B))]).astype(np.int64)
    z = np.zeros(B, dtype=np.int32)
    pl = eng.HostPileup(B, S, cpo, cro, None, nrd, reads, z, z, z)

    def run(env, want):
        monkeypatch.setenv("DMX_EXPERIMENTS", "1")
        for k in ("DMX_K1_CANP", "DMX_K1_NO_CANP", "DMX_K1_CANP_MINW4"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = eng.Engine(V, (0.0, 0.5), 0.5)
        e.set_genotypes(g); e.set_pileup(pl); e.run_singlet(); e.sync()
        assert e.kernel_names()["singlet"].startswith(want), e.kernel_names()
        llks, llk0s = e.get_singlet()
        e.close()
        return llks, llk0s

    base = run({"DMX_K1_NO_CANP": "1"}, "k_singlet_can<")
    for env in ({"DMX_K1_CANP": "1"}, {"DMX_K1_CANP": "1", "DMX_K1_CANP_MINW4": "1"}, {"DMX_K1_CANP": "1"}):
        got = run(env, "k_singlet_canp<")
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), env
    # the oracle on the same pileup (K1 only)
    words = ((reads >> 7).astype(np.uint32) << 24) | ((reads & 0x7F).astype(np.uint32) << 16) | 1
    pair_snp = np.concatenate([np.arange(n, dtype=np.int32) for n in npair]) if P else np.zeros(0, np.int32)
    csr = oracle.Csr([f"c{i:06d}" for i in range(B)], cpo, pair_snp, np.concatenate([[0], np.cumsum(nrd.astype(np.int64))]), words.astype(np.uint32), z, z, z)
    ref = oracle.run_csr(csr, [f"s{j}" for j in range(V)], g, oracle.Params((0.0, 0.5), 0.5), None, True)
    assert np.abs(base[0] - ref.llks).max() < TOL and np.abs(base[1] - ref.llk0s).max() < TOL


@pytest.mark.parametrize("dense,field", [(True, "GP"), (False, "GP"), (False, "PL")])
def test_symmetric_strict_kernel_gives_k_doublet_a2s_bits(eng, oracle, monkeypatch, dense, field):
    """Round 6 (an experiment kernel, DMX_A2_SYM=1; not faster than k_doublet_a2): k_doublet_a2s (STRICT, default grid, 32 soft-field samples —
    cfg3's shape): one lane owns the entries [j][k] and [k][j] and forms the products
    they share once — the exact g_j[l] g_k[m], and at alpha 0.5 (symmetric mixture) the nine terms themselves, which the reference adds row-major for one
    entry and column-major for the other.  Every operation is the reference's on its operands in its order: the grid, llks00 and the K3 records must equal
    k_doublet_a2's bit for bit — pairs of 0..6 reads and beyond kSafeReads, whole-range base qualities, tiles with and without a
    deep pair (the final-value table on and off), ragged last sub-tiles — and agree with the oracle."""
    from demuxlet_amd import synth, capi
    V = 32
    g, pl = _mixed_depth_problem(eng, V, dense)
    if field == "PL":
        rng = np.random.default_rng(4242)
        raw = synth.make_raw_genotypes(rng, g.shape[0], V)
        g = np.stack([eng.geno_from_pl(x) for x in synth.raw_pl_from_alleles(rng, raw.alleles)])
    first = _grid_with_env(eng, monkeypatch, g, pl, V, capi.DMX_MODE_STRICT, {}, "k_doublet_a2u<")   # (before k_doublet_a2 has left its results in any buffer)
    base = _grid_with_env(eng, monkeypatch, g, pl, V, capi.DMX_MODE_STRICT, {"DMX_A2_NO_SYMU": "1"}, "k_doublet_a2<")
    assert np.array_equal(first[0], base[0]) and np.array_equal(first[1], base[1])
    # the shipped form: k_doublet_a2's kernel over unordered pairs (k_doublet_a2u) + the diagonal entries (k_doublet_diag) behind it
    for env in ({}, {"DMX_A2_NO_FINALS": "1"}, {"DMX_FINALS_ANY_DEPTH": "1"}, {"DMX_A2_NO_SEEDS": "1", "DMX_A2_NO_FINALS": "1"}):
        got = _grid_with_env(eng, monkeypatch, g, pl, V, capi.DMX_MODE_STRICT, env, "k_doublet_a2u<")
        assert np.array_equal(got[0], base[0]), (env, np.argwhere(got[0] != base[0])[:5])
        assert np.array_equal(got[1], base[1]), env
    # the one-wavefront-per-(barcode, slab) experiment kernel
    for env in ({"DMX_A2_SYM": "1"}, {"DMX_A2_SYM": "1", "DMX_A2_NO_FINALS": "1"}, {"DMX_A2_SYM": "1", "DMX_FINALS_ANY_DEPTH": "1"}, {"DMX_A2_SYM": "1", "DMX_A2S_MINW4": "1"}):
        got = _grid_with_env(eng, monkeypatch, g, pl, V, capi.DMX_MODE_STRICT, env, "k_doublet_a2s<")
        assert np.array_equal(got[0], base[0]), (env, np.argwhere(got[0] != base[0])[:5])
        assert np.array_equal(got[1], base[1]), env
    # the oracle on the same pileup
    B, S = pl.n_cells, pl.n_snps
    words = ((pl.reads >> 7).astype(np.uint32) << 24) | ((pl.reads & 0x7F).astype(np.uint32) << 16) | 1
    pair_snp = pl.pair_snp if pl.pair_snp is not None else np.tile(np.arange(S, dtype=np.int32), B)
    z = np.zeros(B, dtype=np.int32)
    csr = oracle.Csr([f"c{i:06d}" for i in range(B)], pl.cell_pair_off, pair_snp, np.concatenate([[0], np.cumsum(pl.pair_nrd.astype(np.int64))]),
                     words.astype(np.uint32), z, z, z)
    ref = oracle.run_csr(csr, [f"s{j}" for j in range(V)], g, oracle.Params((0.0, 0.5), 0.5), None, False)
    proc = ref.processed.astype(bool)
    assert np.abs(base[0][proc] - ref.llksAB[proc]).max() < TOL


@pytest.mark.parametrize("V", [32, 16])
@pytest.mark.parametrize("B,S,cover", [(5, 45, 0.5), (1, 31, 1.0), (9, 333, 0.08), (130, 64, 0.3), (37, 700, 1.0), (41, 900, 0.35)])
def test_unordered_pair_kernel_on_ragged_small_problems(eng, monkeypatch, B, S, cover, V):
    """k_doublet_a2u (32 samples) / k_doublet_a2u16 (16) + their diagonal kernel on the shapes the big tests do not reach: barcode counts that are not multiples of 4 (the diagonal kernel's
    workgroups hold four barcodes), barcodes without any covered SNP, fewer pairs than a tile or a sub-tile, a single barcode — bit for bit k_doublet_a2's grid,
    llks00 and K3 records."""
    from demuxlet_amd import synth, capi
    rng = np.random.default_rng(6100 + B + S + V)
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([eng.geno_from_gp(x, 0.01) for x in synth.raw_gp_from_alleles(rng, raw.alleles)])
    cov = rng.random((B, S)) < cover
    if B > 2:
        cov[1, :] = False                                                 # a barcode without a pair
    if cover >= 1.0:
        cov[:] = True
    npair = cov.sum(axis=1)
    dense = bool(cov.all())
    pair_snp = None if dense else np.concatenate([np.nonzero(cov[c])[0] for c in range(B)]).astype(np.int32)
    P = int(npair.sum())
    nrd = rng.choice(np.arange(7), size=P, p=[0.1, 0.55, 0.2, 0.07, 0.04, 0.02, 0.02]).astype(np.uint8)
    if P > 100:
        nrd[rng.random(P) < 0.003] = 20                                   # beyond kSafeReads
    nr = int(nrd.sum())
    reads = (rng.integers(2, 70, size=nr).astype(np.uint8)) | (rng.integers(0, 2, size=nr).astype(np.uint8) << 7)
    cpo = np.concatenate([[0], np.cumsum(npair)]).astype(np.int64)
    cro = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(B), npair), weights=nrd, minlength=B))]).astype(np.int64)
    z = np.zeros(B, dtype=np.int32)
    pl = eng.HostPileup(B, S, cpo, cro, pair_snp, nrd, reads, z, z, z)

    def run(env, want):
        monkeypatch.setenv("DMX_EXPERIMENTS", "1")
        for k in ("DMX_A2_NO_SYMU", "DMX_FINALS_ANY_DEPTH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = eng.Engine(V, (0.0, 0.5), 0.5)
        e.set_genotypes(g); e.set_pileup(pl); e.run(); e.sync()
        assert e.kernel_names()["doublet"].startswith(want), e.kernel_names()
        out = e.get_doublet()
        e.close()
        return out

    # (the unordered-pair kernel FIRST: its buffers must not hold a previous run's identical results where it fails to write)
    bs = [run(env, "k_doublet_a2u") for env in ({}, {"DMX_FINALS_ANY_DEPTH": "1"})]
    a = run({"DMX_A2_NO_SYMU": "1"}, "k_doublet_a2<")
    for env, b in zip(({}, {"DMX_FINALS_ANY_DEPTH": "1"}), bs):
        covered = npair > 0
        assert np.array_equal(a[0][covered], b[0][covered]) and np.array_equal(a[1][covered], b[1][covered]), env
        assert a[2].tobytes() == b[2].tobytes(), env
