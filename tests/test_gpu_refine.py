"""GPU (-m gpu): genotype refinement from called singlets (Engine.refine_genotypes / dmx_engine_refine_genotypes, refine.refine_run).

LL and the counts are checked against a float64 numpy restatement of cmd_cram_demuxlet.cpp:426-452 (the per-pair GL vector after the
+1e-6 renormalisation, summed with np.log in plain barcode order): |d| <= 1e-9, counts exact; gp' within 2 float32 ulp of the numpy
posterior, uncovered rows the prior's bits.  Then determinism, no interference with the engine's other results, the device hand-off,
two full-size shapes (cfg3 dense, cfg6 sparse) on sampled rows, and that the refinement does what it is for."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-9
C = 64          # the contract's chunk of assigned barcodes


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import build, capi, engine, refine, synth, synth_torch
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return dict(torch=torch, capi=capi, engine=engine, refine=refine, synth=synth, st=synth_torch)


def pair_gl(nrd, start, reads, mat, err):
    """float64 [P][3]: :427-452 for every pair (reads in stored order), vectorised over pairs."""
    P = len(nrd)
    G = np.ones((P, 3))
    e3_of, het_of = err / 3.0, 0.5 - err / 3.0
    for r in range(int(nrd.max()) if P else 0):
        idx = np.flatnonzero(nrd > r)
        b = reads[start[idx] + r].astype(np.int64)
        bq, alt = b & 127, (b >> 7) != 0
        m_, e3, h = mat[bq], e3_of[bq], het_of[bq]
        g0 = G[idx, 0] * np.where(alt, e3, m_)
        g1 = G[idx, 1] * h
        g2 = G[idx, 2] * np.where(alt, m_, e3)
        tmp = g0 + g1 + g2
        G[idx, 0], G[idx, 1], G[idx, 2] = g0 / tmp, g1 / tmp, g2 / tmp
    G = G + 1e-6
    tmp = G[:, 0] + G[:, 1] + G[:, 2]
    return G / tmp[:, None]


def alt_counts(nrd, start, reads):
    alt = np.zeros(len(nrd), dtype=np.int64)
    for r in range(int(nrd.max()) if len(nrd) else 0):
        idx = np.flatnonzero(nrd > r)
        alt[idx] += reads[start[idx] + r] >> 7
    return alt


def ref_refine(cell, snp, nrd, start, reads, assign, S, V, mat, err):
    """LL[S][V][3], n_cell / n_ref / n_alt [S][V] over the pairs given (cell ascending), np.log, plain barcode order."""
    keep = assign[cell] >= 0
    cell, snp, nrd, start = cell[keep], snp[keep], nrd[keep].astype(np.int64), start[keep]
    gl = pair_gl(nrd, start, reads, mat, err)
    alt = alt_counts(nrd, start, reads)
    v = assign[cell]
    LL = np.zeros((S, V, 3))
    for g in range(3):
        np.add.at(LL[:, :, g], (snp, v), np.log(gl[:, g]))
    n_cell, n_ref, n_alt = (np.zeros((S, V), dtype=np.int64) for _ in range(3))
    np.add.at(n_cell, (snp, v), 1)
    np.add.at(n_ref, (snp, v), nrd - alt)
    np.add.at(n_alt, (snp, v), alt)
    return LL, n_cell, n_ref, n_alt


def ref_posterior(LL, n_cell, prior, floor):
    q = prior.astype(np.float64) + floor
    w = q * np.exp(LL - LL.max(axis=2, keepdims=True))
    post = (w / w.sum(axis=2, keepdims=True)).astype(np.float32)
    return np.where((n_cell > 0)[..., None], post, prior)


def host_pairs(sp):
    B = sp.n_cells
    po = np.asarray(sp.cell_pair_off, dtype=np.int64)
    cell = np.repeat(np.arange(B), np.diff(po))
    snp = np.asarray(sp.pair_snp, dtype=np.int64) if sp.pair_snp is not None else np.arange(len(cell)) - po[cell]
    nrd = np.asarray(sp.pair_nrd, dtype=np.int64)
    start = np.cumsum(nrd) - nrd
    assert np.array_equal(start[po[:-1][np.diff(po) > 0]], np.asarray(sp.cell_read_off)[:-1][np.diff(po) > 0])
    return cell, snp, nrd, start


def host_pileup(m, sp):
    return m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads,
                                  sp.rd_totl, sp.rd_pass, sp.rd_uniq)


def make_prior(m, rng, raw, field):
    eng, synth = m["engine"], m["synth"]
    S = raw.alleles.shape[0]
    if field == "GT":
        return np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    gp = synth.raw_gp_from_alleles(rng, raw.alleles, soft=0.3)
    return np.stack([eng.geno_from_gp(gp[s], 0.01) for s in range(S)])


def check(m, sp, g, assign, floor=1e-3, eng=None):
    V, S = g.shape[1], g.shape[0]
    mat, err = m["engine"].phred_tables()
    own = eng is None
    if own:
        eng = m["engine"].Engine(V, (0.0, 0.5), 0.5)
        eng.set_genotypes(g); eng.set_pileup(host_pileup(m, sp))
    try:
        ll, n_cell, n_ref, n_alt, gp = eng.refine_genotypes(assign, g, floor)
        info = eng.refine_info()
    finally:
        if own:
            eng.close()
    cell, snp, nrd, start = host_pairs(sp)
    LL, nc, nr, na = ref_refine(cell, snp, nrd, start, np.asarray(sp.reads), np.asarray(assign), S, V, mat, err)
    assert np.array_equal(n_cell, nc) and np.array_equal(n_ref, nr) and np.array_equal(n_alt, na)
    d = np.abs(ll - LL).max() if ll.size else 0.0
    assert d <= TOL, d
    want = ref_posterior(LL, nc, g, floor)
    cov = nc > 0
    ulp = np.abs(gp.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulp[cov].max(initial=0) <= 2
    assert np.array_equal(gp[~cov].view(np.uint32), g[~cov].view(np.uint32))
    return ll, n_cell, gp, info


@pytest.mark.parametrize("B,S,V,delta,rbar,dense,field", [
    (300, 257, 8, 1.0, 1.25, True, "GP"),        # dense layout
    (200, 700, 2, 0.2, 1.5, False, "GT"),        # V = 2
    (240, 900, 16, 0.05, 2.0, False, "GP"),      # sparse, cfg5-like
    (260, 400, 32, 0.3, 1.0, False, "GP"),       # one read per pair: many pairs with 0 stored reads
    (400, 300, 64, 0.002, 1.5, False, "GT"),     # most barcodes have no pair at all
])
def test_refine_parity(m, B, S, V, delta, rbar, dense, field):
    rng = np.random.default_rng(B * 7 + S + V)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = make_prior(m, rng, raw, field)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, delta, rbar, dense_layout=dense)
    assert (sp.pair_snp is None) == dense
    if rbar == 1.0:
        assert (np.asarray(sp.pair_nrd) == 0).any()
    if delta < 0.01:
        assert (np.diff(sp.cell_pair_off) == 0).sum() > B // 2
    assign = sp.truth[:, 0].copy()
    assign[sp.truth[:, 1] >= 0] = -1            # doublets are not used
    assign[assign == 1] = -1                    # a sample with no assigned barcode
    check(m, sp, g, assign)


def test_refine_deep_pairs_u16(m):
    rng = np.random.default_rng(17)
    S, V, B = 60, 4, 24
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = make_prior(m, rng, raw, "GP")
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.4, 300.0)
    assert sp.pair_nrd.dtype == np.uint16 and int(sp.pair_nrd.max()) > 255
    check(m, sp, g, sp.truth[:, 0].copy())


def test_refine_chunk_boundaries_and_unassigned(m):
    """One sample with exactly C assigned barcodes, one with C + 1, one with 1; then assign = -1 everywhere."""
    rng = np.random.default_rng(23)
    S, V, B = 500, 8, 3 * C + 40
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = make_prior(m, rng, raw, "GT")
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.1, 1.5)
    perm = rng.permutation(B)
    assign = np.full(B, -1, dtype=np.int32)
    assign[perm[:C]] = 0
    assign[perm[C:2 * C + 1]] = 3
    assign[perm[2 * C + 1]] = 5
    assign[perm[2 * C + 2:]] = rng.choice(np.array([-1, 1, 2, 4, 6, 7], dtype=np.int32), size=B - 2 * C - 2)
    assert (assign == 0).sum() == C and (assign == 3).sum() == C + 1 and (assign == 5).sum() == 1
    _, _, _, info = check(m, sp, g, assign)
    assert info["chunk_cells"] == C
    ll, n_cell, gp, info = check(m, sp, g, np.full(B, -1, dtype=np.int32))
    assert info["n_chunks"] == 0 and not n_cell.any() and not ll.any()
    assert np.array_equal(gp.view(np.uint32), g.view(np.uint32))


def test_refine_determinism_and_no_interference(m):
    eng = m["engine"]
    rng = np.random.default_rng(29)
    S, V, B = 800, 8, 300
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = make_prior(m, rng, raw, "GP")
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.2, 1.5)
    pl = host_pileup(m, sp)
    assign = sp.truth[:, 0].copy()

    def results(e):
        llks, llk0s = e.get_singlet()
        grid, l00, summ = e.get_doublet()
        return [llks, llk0s, grid, l00, summ.view(np.uint8)]

    a = eng.Engine(V, (0.0, 0.5), 0.5)
    a.set_genotypes(g); a.set_pileup(pl); a.run(); a.sync()
    base = results(a)
    a.close()
    b = eng.Engine(V, (0.0, 0.5), 0.5)
    b.set_genotypes(g); b.set_pileup(pl)
    r1 = b.refine_genotypes(assign, g)
    r2 = b.refine_genotypes(assign, g)
    b.run(); b.sync()
    r3 = b.refine_genotypes(assign, g)
    after = results(b)
    b.close()
    for x, y, z in zip(r1, r2, r3):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) and np.array_equal(x.view(np.uint8), z.view(np.uint8))
    for x, y in zip(base, after):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_refine_device_hand_off(m):
    eng = m["engine"]
    rng = np.random.default_rng(31)
    S, V, B = 600, 8, 200
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = make_prior(m, rng, raw, "GP")
    for dense in (False, True):
        sp = m["synth"].make_pileup(rng, raw.alleles, B, 1.0 if dense else 0.2, 1.3, dense_layout=dense)
        pl = host_pileup(m, sp)
        a = eng.Engine(V, (0.0, 0.5), 0.5)
        a.set_genotypes(g); a.set_pileup(pl)
        gp = a.refine_genotypes(sp.truth[:, 0].copy(), g)[4]
        a.set_genotypes_device(a.refined_device_ptr(), S)
        a.set_pileup(pl)
        a.run_singlet(); a.sync()
        dev = a.get_singlet()
        b = eng.Engine(V, (0.0, 0.5), 0.5)
        b.set_genotypes(gp); b.set_pileup(pl); b.run_singlet(); b.sync()
        host = b.get_singlet()
        a.refine_genotypes(sp.truth[:, 0].copy(), g)        # a second refinement does not overwrite the matrix the engine holds
        a.run_singlet(); a.sync()
        again = a.get_singlet()
        a.close(); b.close()
        for x, y, z in zip(dev, host, again):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)) and np.array_equal(x.view(np.uint64), z.view(np.uint64))


@pytest.mark.parametrize("cfg_id", [3, 6])
def test_refine_full_size(m, cfg_id):
    """cfg3 (dense, 10k x 50k x 32, GP) and cfg6 (sparse 10x-like, 20k x 100k x 16): every barcode assigned from truth; parity on
    a sample of SNPs (every sample's row there) against numpy over the barcodes involved."""
    torch, eng = m["torch"], m["engine"]
    import bench
    cfg = bench.CONFIGS[cfg_id]
    B, S, V = cfg["B"], cfg["S"], cfg["V"]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0xD3A00000 + cfg_id)
    raw, g = bench.genotype_matrix(eng, m["synth"], rng, S, V, cfg["field"])
    dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
    dp = m["st"].make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xD3A0 + 1000 * cfg_id, device=dev)
    assign = dp.truth[:, 0].contiguous()
    e = eng.Engine(V, cfg["alphas"], 0.5)
    e.set_genotypes(g)
    e.set_pileup_struct(dp.as_struct(), keep=dp)
    ll, n_cell, n_ref, n_alt, gp = e.refine_genotypes(int(assign.data_ptr()), g)      # assign in device memory
    info = e.refine_info()
    e.close()
    sel = np.unique(np.concatenate([[0, S - 1], rng.choice(S, 30, replace=False)])).astype(np.int64)
    po = dp.cell_pair_off
    if dp.pair_snp is None:
        cells = torch.arange(B, device=dev).repeat_interleave(len(sel))
        pidx = po[:-1].repeat_interleave(len(sel)) + torch.from_numpy(sel).to(dev).repeat(B)
        snp = torch.from_numpy(sel).to(dev).repeat(B)
    else:
        hit = torch.isin(dp.pair_snp, torch.from_numpy(sel).to(dev).to(torch.int32))
        pidx = torch.nonzero(hit).flatten()
        cells = torch.searchsorted(po, pidx, right=True) - 1
        snp = dp.pair_snp[pidx].to(torch.int64)
    cum = torch.cumsum(dp.pair_nrd.to(torch.int64), 0)
    nrd = dp.pair_nrd[pidx].to(torch.int64)
    start_g = cum[pidx] - nrd
    del cum
    mx = int(nrd.max().item())
    ridx = (start_g[:, None] + torch.arange(max(mx, 1), device=dev)[None, :]).clamp(max=max(dp.n_reads - 1, 0))
    rd = dp.reads[ridx].cpu().numpy().reshape(-1)
    n = len(pidx)
    start = np.arange(n, dtype=np.int64) * max(mx, 1)
    mat, err = eng.phred_tables()
    LL, nc, nr, na = ref_refine(cells.cpu().numpy(), snp.cpu().numpy(), nrd.cpu().numpy(), start, rd, assign.cpu().numpy(), S, V, mat, err)
    assert np.array_equal(n_cell[sel], nc[sel]) and np.array_equal(n_ref[sel], nr[sel]) and np.array_equal(n_alt[sel], na[sel])
    assert nc[sel].sum() > 0
    d = np.abs(ll[sel] - LL[sel]).max()
    assert d <= TOL, d
    want = ref_posterior(LL[sel], nc[sel], g[sel], 1e-3)
    cov = nc[sel] > 0
    ulp = np.abs(gp[sel].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulp[cov].max(initial=0) <= 2
    assert info["n_assigned"] == B and info["n_chunks"] == sum(-(-int((dp.truth[:, 0] == v).sum()) // C) for v in range(V))


def corrupt(rng, g, samples, frac):
    S = g.shape[0]
    rows = {0: np.array([0.99, 0.005, 0.005]), 1: np.array([0.005, 0.99, 0.005]), 2: np.array([0.005, 0.005, 0.99])}
    bad = g.copy()
    for v in samples:
        idx = rng.choice(S, int(frac * S), replace=False)
        for i in idx:
            bad[i, v] = rows[int(rng.integers(0, 3))].astype(np.float32)
    return bad


def test_refine_recovers_corrupted_genotypes(m):
    """Two samples' priors are wrong at 40 % of the SNPs; one refinement from truth-derived singlets puts the argmax back on the true
    genotype at covered SNPs clearly more often than the corrupted prior."""
    rng = np.random.default_rng(41)
    S, V, B = 2000, 8, 800
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = make_prior(m, rng, raw, "GT")
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.3, 1.5)
    bad = corrupt(rng, g, (0, 1), 0.4)
    assign = sp.truth[:, 0].copy()
    assign[sp.truth[:, 1] >= 0] = -1
    _, n_cell, gp, _ = check(m, sp, bad, assign)
    gt = np.clip(raw.alleles, 0, 1).sum(axis=2)
    for v in (0, 1):
        cov = n_cell[:, v] > 0
        acc_prior = (bad[cov, v].argmax(axis=1) == gt[cov, v]).mean()
        acc_ref = (gp[cov, v].argmax(axis=1) == gt[cov, v]).mean()
        assert cov.sum() > S // 2
        assert acc_ref >= acc_prior + 0.15, (v, acc_prior, acc_ref)


def test_refine_run_rounds(m, tmp_path):
    """refine_run: rounds = 0 writes exactly what demuxlet_run writes; one round with the refined matrix calls at least as many barcodes
    correctly as round 0 on a panel whose VCF rows are corrupted for two samples."""
    eng, refine = m["engine"], m["refine"]
    rng = np.random.default_rng(43)
    S, V, B = 3000, 8, 1200
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = make_prior(m, rng, raw, "GT")
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.04, 1.5)
    bad = corrupt(rng, g, (0, 1), 0.6)
    pl = host_pileup(m, sp)
    samples = [f"S-{j}" for j in range(V)]
    barcodes = [m["synth"].barcode_name(c) for c in range(B)]
    eng.demuxlet_run(pl, bad, samples, (0.0, 0.5), str(tmp_path / "plain"), barcodes=barcodes)
    refine.refine_run(pl, bad, samples, (0.0, 0.5), str(tmp_path / "r0"), rounds=0, barcodes=barcodes)
    for ext in (".best", ".single", ".sing2"):
        assert (tmp_path / ("plain" + ext)).read_bytes() == (tmp_path / ("r0" + ext)).read_bytes()
    assert not (tmp_path / "r0.refined.tsv").exists()
    refine.refine_run(pl, bad, samples, (0.0, 0.5), str(tmp_path / "o"), rounds=1, barcodes=barcodes)

    def correct(prefix):
        a = refine.assignments_from_best(str(tmp_path / (prefix + ".best")), samples, barcodes)
        sng = sp.truth[:, 1] < 0
        return int(((a == sp.truth[:, 0]) & sng).sum())

    c0, c1 = correct("o"), correct("o.r1")
    assert c1 >= c0, (c0, c1)
    lines = (tmp_path / "o.refined.tsv").read_text().splitlines()
    assert lines[0].startswith("RID\tPOS\tREF\tALT\tSM_ID\tN.CELL") and len(lines) > S


@pytest.mark.parametrize("quals", ["full", "edges", "max"])
@pytest.mark.parametrize("field", ["GT", "GP"])
def test_refine_parity_quality_range(m, field, quals):
    """Base qualities over 0..127 (the 0.75 error floor at q <= 1, err(127)) and the depth mix of tests/quality_mix.py: 0..6, 14..17 (both
    sides of kSafeReads), 40 and u16 pairs of 256..300 reads, a share of them all-ALT on hom-REF rows (or the reverse)."""
    from quality_mix import mixed_depth_pileup
    rng = np.random.default_rng(8800 + len(field) + {"full": 0, "edges": 1, "max": 2}[quals])
    S, V, B = 400, 8, 200
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = make_prior(m, rng, raw, field)
    sp = mixed_depth_pileup(rng, raw.alleles, B, 0.2, quals=quals, deep=4)
    assert sp.pair_nrd.dtype == np.uint16
    assign = sp.truth[:, 0].copy()
    assign[sp.truth[:, 1] >= 0] = -1
    check(m, sp, g, assign)
