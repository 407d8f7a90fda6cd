"""GPU (-m gpu): the ambient contamination profile (Engine.ambient_profile / dmx_engine_ambient, ambient.ambient_run).

LL is checked against the float64 numpy restatement of tests/ambient_ref.py (logsumexp over g of log gp + the summed log read factors,
each barcode's terms added serially): |d| <= 1e-9, N.SNP / N.READ exact.  Then determinism (repeat, grid split, host vs device assign),
no interference with the engine's other results, recovery of the contamination on synthetic pools, two full-size shapes on sampled
barcodes, and the command line end to end."""
import json
import os

import numpy as np
import pytest

import ambient_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import ambient, build, capi, engine, refine, synth, synth_torch
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return dict(torch=torch, capi=capi, engine=engine, refine=refine, synth=synth, st=synth_torch, ambient=ambient)


def host_pileup(m, sp, width=None):
    nrd = np.asarray(sp.pair_nrd)
    if width is not None:
        nrd = nrd.astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[width])
    return m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, nrd, sp.reads,
                                  sp.rd_totl, sp.rd_pass, sp.rd_uniq)


def gt_matrix(m, raw):
    S = raw.alleles.shape[0]
    return np.stack([m["engine"].geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])


def make_grid(Q):
    if Q == 1:
        return np.array([0.15])
    return np.linspace(0.0, 1.0, Q)                 # contains 0 and 1


def run_profile(m, g, pl, assign, a, grid):
    V = g.shape[1]
    e = m["engine"].Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        out = e.ambient_profile(assign, a, grid)
        info = e.ambient_info()
    finally:
        e.close()
    return out, info


def check(m, sp, g, assign, a, grid, width=None):
    pl = host_pileup(m, sp, width)
    (ll, n_snp, n_read), info = run_profile(m, g, pl, assign, a, grid)
    mat, err = m["engine"].phred_tables()
    LL, ns, nr = R.ref_profile(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, assign, g, a, grid, mat, err)
    assert np.array_equal(n_snp, ns) and np.array_equal(n_read, nr)
    d = np.abs(ll - LL).max() if ll.size else 0.0
    assert d <= TOL, d
    assert not ll[np.asarray(assign) < 0].any()
    assert info["n_grid"] == len(grid) and info["n_cells"] == sp.n_cells and info["n_assigned"] == int((np.asarray(assign) >= 0).sum())
    return ll, n_snp, n_read


@pytest.mark.parametrize("B,S,V,delta,rbar,dense,width,Q", [
    (150, 257, 8, 1.0, 1.25, True, 1, 51),          # dense
    (140, 257, 4, 1.0, 1.5, True, 4, 65),           # dense, u32 read counts, two grid blocks
    (200, 900, 16, 0.05, 2.0, False, 2, 64),        # sparse, u16 read counts, one full grid block
    (260, 400, 32, 0.3, 1.0, False, 1, 256),        # one read per pair: many pairs with no stored read; the longest grid
    (300, 300, 8, 0.002, 1.5, False, 1, 1),         # many barcodes have no pair at all; one grid point
])
def test_ambient_parity(m, B, S, V, delta, rbar, dense, width, Q):
    rng = np.random.default_rng(B * 11 + S + V + Q)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    g[rng.choice(S, S // 10, replace=False), rng.integers(0, V)] = 0.0               # all-zero rows
    hard = rng.choice(S, S // 10, replace=False)
    g[hard, 0] = np.array([1.0, 0.0, 0.0], dtype=np.float32)                        # rows with hard zeros
    rho = rng.choice([0.0, 0.1, 0.3], size=B)
    sp, _, a = m["synth"].make_ambient_pileup(rng, raw.alleles, B, delta, rbar, rho, dense_layout=dense)
    assert (sp.pair_snp is None) == dense
    a = a.copy()
    a[rng.choice(S, S // 8, replace=False)] = 0.0
    a[rng.choice(S, S // 8, replace=False)] = 1.0
    if rbar == 1.0:
        assert (np.asarray(sp.pair_nrd) == 0).any()
    if delta < 0.01:
        assert (np.diff(sp.cell_pair_off) == 0).sum() > B // 4
    assign = sp.truth[:, 0].copy()
    assign[rng.random(B) < 0.2] = -1                                                # unassigned barcodes
    check(m, sp, g, assign, a, make_grid(Q), width)


def deep_pileup(m, rng, S, V):
    """Four barcodes; barcode 1 also has, at SNP 5, one pair of 3 200 stored reads (u16 counts), 90 % ALT at bq 40 on a hom-REF row with
    hard zeros: its plain float64 product underflows at small rho."""
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    sp = m["synth"].make_pileup(rng, raw.alleles, 4, 0.3, 1.5, doublet_rate=0.0)
    _, snp, nrd, start = R.host_pairs(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd)
    po = np.asarray(sp.cell_pair_off)
    cells = [[(int(snp[k]), np.asarray(sp.reads)[start[k]:start[k] + nrd[k]]) for k in range(po[c], po[c + 1]) if snp[k] != 5] for c in range(4)]
    deep = np.where(rng.random(3200) < 0.9, (1 << 7) | 40, 35).astype(np.uint8)
    cells[1] = sorted(cells[1] + [(5, deep)], key=lambda x: x[0])
    pairs = [p for c in cells for p in c]
    po = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.int64)
    ro = np.concatenate([[0], np.cumsum([sum(len(r) for _, r in c) for c in cells])]).astype(np.int64)
    t = np.ones(4, dtype=np.int32)
    sp2 = m["synth"].SynthPileup(4, S, po, ro, np.array([s for s, _ in pairs], dtype=np.int32), np.array([len(r) for _, r in pairs], dtype=np.uint16),
                                 np.concatenate([r for _, r in pairs]).astype(np.uint8), t, t, t,
                                 np.stack([np.arange(4) % V, np.full(4, -1)], axis=1).astype(np.int32))
    g = gt_matrix(m, raw)
    g[5, :] = np.array([1.0, 0.0, 0.0], dtype=np.float32)
    return sp2, g


def test_ambient_deep_pair(m):
    rng = np.random.default_rng(17)
    S, V = 60, 4
    sp, g = deep_pileup(m, rng, S, V)
    a = rng.uniform(0.05, 0.95, size=S)
    grid = np.array([0.0, 1e-3, 0.01, 0.05, 0.2, 0.5, 0.9, 1.0])
    ll, n_snp, n_read = check(m, sp, g, np.arange(4, dtype=np.int32) % V, a, grid)
    assert ll[1, 0] < -20000 and np.isfinite(ll[1]).all()


def test_ambient_determinism(m):
    eng = m["engine"]
    rng = np.random.default_rng(29)
    S, V, B = 800, 8, 300
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp, _, a = m["synth"].make_ambient_pileup(rng, raw.alleles, B, 0.2, 1.5, rng.choice([0.0, 0.2], size=B))
    pl = host_pileup(m, sp)
    assign = sp.truth[:, 0].copy()
    assign[::7] = -1
    grid = np.linspace(0.0, 1.0, 128)
    torch = m["torch"]
    d_assign = torch.from_numpy(assign).to("cuda:0")
    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        r1 = e.ambient_profile(assign, a, grid)
        r2 = e.ambient_profile(assign, a, grid)
        lo = e.ambient_profile(assign, a, grid[:64])
        hi = e.ambient_profile(assign, a, grid[64:])
        dv = e.ambient_profile(int(d_assign.data_ptr()), a, grid)
    finally:
        e.close()
    for x, y in ((r1, r2), (r1, dv)):
        for u, w in zip(x, y):
            assert np.array_equal(u.view(np.uint8), w.view(np.uint8))
    split = np.concatenate([lo[0], hi[0]], axis=1)
    assert np.array_equal(r1[0].view(np.uint64), split.view(np.uint64))
    assert np.array_equal(lo[1], r1[1]) and np.array_equal(hi[2], r1[2])


def test_ambient_no_interference(m):
    eng = m["engine"]
    rng = np.random.default_rng(31)
    S, V, B = 700, 8, 260
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp, _, a = m["synth"].make_ambient_pileup(rng, raw.alleles, B, 0.2, 1.4, 0.1)
    pl = host_pileup(m, sp)
    assign = sp.truth[:, 0].copy()
    grid = m["ambient"].default_grid()

    def results(e):
        llks, llk0s = e.get_singlet()
        grid_, l00, summ = e.get_doublet()
        return [llks, llk0s, grid_, l00, summ.view(np.uint8)]

    x = eng.Engine(V, (0.0, 0.5), 0.5)
    x.set_genotypes(g); x.set_pileup(pl)
    x.run(); x.sync()
    base = results(x)
    ref0 = x.refine_genotypes(assign, g)
    x.close()
    y = eng.Engine(V, (0.0, 0.5), 0.5)
    y.set_genotypes(g); y.set_pileup(pl)
    p0 = y.ambient_profile(assign, a, grid)
    y.run(); y.sync()
    p1 = y.ambient_profile(assign, a, grid)
    after = results(y)
    ref1 = y.refine_genotypes(assign, g)
    p2 = y.ambient_profile(assign, a, grid)
    ref2 = y.refine_genotypes(assign, g)
    after2 = results(y)
    y.close()
    for u, w in zip(base, after):
        assert np.array_equal(u.view(np.uint8), w.view(np.uint8))
    for u, w in zip(base, after2):
        assert np.array_equal(u.view(np.uint8), w.view(np.uint8))
    for r in (ref1, ref2):
        for u, w in zip(ref0, r):
            assert np.array_equal(u.view(np.uint8), w.view(np.uint8))
    for p in (p1, p2):
        for u, w in zip(p0, p):
            assert np.array_equal(u.view(np.uint8), w.view(np.uint8))


def test_ambient_argument_errors(m):
    capi, eng = m["capi"], m["engine"]
    rng = np.random.default_rng(37)
    S, V, B = 100, 4, 20
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp, _, a = m["synth"].make_ambient_pileup(rng, raw.alleles, B, 0.3, 1.2, 0.1)
    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g)
        e.B = B
        with pytest.raises(capi.DmxError) as ei:           # no pileup yet
            e.ambient_profile(np.zeros(B, dtype=np.int32), a, [0.0, 0.1])
        assert ei.value.code == -3
        e.set_pileup(host_pileup(m, sp))
        asg = np.zeros(B, dtype=np.int32)
        for bad_grid in ([], [0.2, 0.1], [0.1, 0.1], [-0.1, 0.2], [0.0, 1.5], list(np.linspace(0, 1, 257))):
            with pytest.raises(capi.DmxError) as ei:
                e.ambient_profile(asg, a, bad_grid)
            assert ei.value.code == -1
        for bad_a in (np.full(S, 1.2), np.full(S, np.nan), a[:-1]):
            with pytest.raises(capi.DmxError) as ei:
                e.ambient_profile(asg, bad_a, [0.0, 0.1])
            assert ei.value.code == -1
        with pytest.raises(capi.DmxError) as ei:
            e.ambient_profile(np.full(B, V, dtype=np.int32), a, [0.0, 0.1])
        assert ei.value.code == -1
        with pytest.raises(ValueError):
            e.ambient_profile(np.zeros(B + 1, dtype=np.int32), a, [0.0, 0.1])
        with pytest.raises(capi.DmxError) as ei:
            capi.check(e._L.dmx_engine_get_ambient(e._h, None, None, None))
        assert ei.value.code == -3                         # nothing computed yet
    finally:
        e.close()


def recovery_pool(m, seed, B, rho, S=20000, V=8, delta=0.1):
    """~2 000 covered SNPs per barcode, rbar 1.25 (cfg6-like depth)."""
    rng = np.random.default_rng(seed)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp, rho, a = m["synth"].make_ambient_pileup(rng, raw.alleles, B, delta, 1.25, rho)
    return sp, g, rho, a


def report(name, **kw):
    d = os.environ.get("DMX_AMBIENT_REPORT")
    if d:
        with open(d, "a") as f:
            f.write(json.dumps(dict(test=name, **kw)) + "\n")


def test_ambient_recovery_per_barcode(m):
    A = m["ambient"]
    levels = np.array([0.0, 0.05, 0.1, 0.2, 0.3])
    B = 600
    rho = levels[np.arange(B) % len(levels)]
    sp, g, rho, a = recovery_pool(m, 41, B, rho)
    grid = A.default_grid()
    (ll, n_snp, _), _ = run_profile(m, g, host_pileup(m, sp), sp.truth[:, 0].copy(), a, grid)
    s = A.summarize(ll, grid)
    med_err = {float(r): float(np.median(np.abs(s.rho[rho == r] - r))) for r in levels}
    med_est = {float(r): float(np.median(s.rho[rho == r])) for r in levels}
    zero_lo = float((s.rho_lo[rho == 0.0] == 0.0).mean())
    covered = (s.rho_lo <= rho) & (rho <= s.rho_hi)
    report("per_barcode", median_snps=float(np.median(n_snp)), median_abs_err=med_err, median_estimate=med_est, rho0_lo_is_0=zero_lo,
           interval_covers_truth=float(covered.mean()))
    assert 1500 < np.median(n_snp) < 2500
    for r in levels:
        assert med_err[float(r)] <= 0.05, (r, med_err)
    assert zero_lo >= 0.8, zero_lo
    assert covered.mean() >= 0.8, covered.mean()


def test_ambient_recovery_pool(m):
    A = m["ambient"]
    res = {}
    for seed, r in ((43, 0.0), (47, 0.1), (53, 0.2)):
        sp, g, _, a = recovery_pool(m, seed, 300, r)
        grid = A.default_grid()
        assign = sp.truth[:, 0].copy()
        (ll, _, _), _ = run_profile(m, g, host_pileup(m, sp), assign, a, grid)
        pool = A.pool_profile(ll, assign)
        res[r] = float(grid[int(np.argmax(pool))])
    report("pool", estimate=res)
    for r, est in res.items():
        assert abs(est - r) <= 0.01 + 1e-12, res


@pytest.mark.parametrize("cfg_id", [3, 6])
def test_ambient_full_size(m, cfg_id):
    """cfg3 (dense, 10k x 50k x 32, GP) and cfg6 (sparse, 20k x 100k x 16): every barcode assigned from truth, 51 grid points; parity
    on sampled barcodes against numpy over their pairs."""
    torch, eng, A = m["torch"], m["engine"], m["ambient"]
    import bench
    cfg = bench.CONFIGS[cfg_id]
    B, S, V = cfg["B"], cfg["S"], cfg["V"]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0xA3B00000 + cfg_id)
    raw, g = bench.genotype_matrix(eng, m["synth"], rng, S, V, cfg["field"])
    dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
    dp = m["st"].make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xA3B0 + 1000 * cfg_id, device=dev)
    assign = dp.truth[:, 0].contiguous()
    a = rng.uniform(0.0, 1.0, size=S)
    grid = A.default_grid()
    e = eng.Engine(V, cfg["alphas"], 0.5)
    e.set_genotypes(g)
    e.set_pileup_struct(dp.as_struct(), keep=dp)
    ll, n_snp, n_read = e.ambient_profile(int(assign.data_ptr()), a, grid)
    info = e.ambient_info()
    e.close()
    assert info["n_assigned"] == B and info["profile_bytes"] == B * len(grid) * 8
    cells = np.unique(np.concatenate([[0, B - 1], rng.choice(B, 4 if cfg_id == 3 else 24, replace=False)]))
    po = dp.cell_pair_off.cpu().numpy()
    ro = dp.cell_read_off.cpu().numpy()
    mat, err = eng.phred_tables()
    asg = assign.cpu().numpy()
    for c in cells:
        p0, p1 = int(po[c]), int(po[c + 1])
        snp = None if dp.pair_snp is None else dp.pair_snp[p0:p1].cpu().numpy()
        nrd = dp.pair_nrd[p0:p1].cpu().numpy()
        reads = dp.reads[int(ro[c]):int(ro[c + 1])].cpu().numpy()
        LL, ns, nr = R.ref_profile(np.array([0, p1 - p0]), snp, nrd, reads, asg[c:c + 1], g, a, grid, mat, err)
        assert ns[0] == n_snp[c] and nr[0] == n_read[c]
        d = np.abs(ll[c] - LL[0]).max()
        assert d <= TOL, (c, d)
    assert n_snp[cells].min() > 0


def test_ambient_cli_end_to_end(m, tmp_path):
    """On a small dump, without --best: the round-0 .best/.single/.sing2 are byte-identical to a plain demuxlet_run, both ambient files
    have the stated columns, and the "reads" ambient builder matches the pooled counts."""
    A, refine, synth, eng = m["ambient"], m["refine"], m["synth"], m["engine"]
    rng = np.random.default_rng(59)
    S, V, B = 1500, 4, 120
    raw = synth.make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp, _, _ = synth.make_ambient_pileup(rng, raw.alleles, B, 0.2, 1.3, rng.choice([0.0, 0.1, 0.25], size=B))
    pl = host_pileup(m, sp)
    samples = [f"S-{j}" for j in range(V)]
    barcodes = [synth.barcode_name(c) for c in range(B)]
    d = refine.PileupDump(samples, [(1, 100 + 10 * j, "A", "C") for j in range(S)], g, barcodes, pl)
    dump = tmp_path / "x.pileup.txt"
    refine.write_pileup_txt(str(dump), d)
    eng.demuxlet_run(pl, g, samples, (0.0, 0.5), str(tmp_path / "plain"), barcodes=barcodes)
    assert A.main(["--pileup", str(dump), "--out", str(tmp_path / "amb")]) == 0
    for ext in (".best", ".single", ".sing2"):
        assert (tmp_path / ("plain" + ext)).read_bytes() == (tmp_path / ("amb" + ext)).read_bytes()
    rows = (tmp_path / "amb.ambient.tsv").read_text().splitlines()
    assert rows[0] == A.AMBIENT_HEADER.rstrip("\n")
    assign = refine.assignments_from_best(str(tmp_path / "plain.best"), samples, barcodes)
    assert len(rows) - 1 == int((assign >= 0).sum()) > B // 2
    assert all(len(r.split("\t")) == 10 for r in rows)
    pool = (tmp_path / "amb.ambient_pool.tsv").read_text().splitlines()
    assert pool[0] == "RHO\tLLK" and len(pool) == 51 + 2 and pool[-1].startswith("#RHO.POOL\t")
    # --best given: no demultiplexing pass, the same profile
    assert A.main(["--pileup", str(dump), "--out", str(tmp_path / "b2"), "--best", str(tmp_path / "plain.best")]) == 0
    assert not (tmp_path / "b2.best").exists()
    assert (tmp_path / "b2.ambient.tsv").read_bytes() == (tmp_path / "amb.ambient.tsv").read_bytes()
    # the "reads" builder: (n_alt + 1) / (n_ref + n_alt + 2) over every barcode's stored reads
    cell, snp, nrd, start = R.host_pairs(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd)
    alt = np.zeros(S); tot = np.zeros(S)
    for k in range(len(cell)):
        r = np.asarray(sp.reads)[start[k]:start[k] + nrd[k]]
        alt[snp[k]] += (r >> 7).sum(); tot[snp[k]] += len(r)
    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        a = A.ambient_from_reads(e, g)
    finally:
        e.close()
    assert np.allclose(a, (alt + 1) / (tot + 2), rtol=0, atol=1e-15)


@pytest.mark.parametrize("quals", ["full", "edges", "max"])
@pytest.mark.parametrize("dense,width", [(False, 2), (True, 1)])
def test_ambient_parity_quality_range(m, dense, width, quals):
    """k_ambient against ambient_ref on reads of quality 0..127 (the 0.75 error floor at q <= 1, err(127)) and soup contamination, then on the
    depth mix of tests/quality_mix.py (0..6, 14..17, 40, u16 pairs of 256..300 reads, all-ALT pairs on hom-REF rows)."""
    from quality_mix import mixed_depth_pileup
    rng = np.random.default_rng(5500 + int(dense) + {"full": 0, "edges": 2, "max": 4}[quals])
    S, V, B = (131, 8, 60) if dense else (600, 16, 120)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    rho = rng.choice([0.0, 0.1, 0.3], size=B)
    sp, _, a = m["synth"].make_ambient_pileup(rng, raw.alleles, B, 1.0 if dense else 0.1, 2.0, rho, dense_layout=dense, quals=quals)
    assign = sp.truth[:, 0].copy()
    assign[rng.random(B) < 0.2] = -1
    check(m, sp, g, assign, a, make_grid(33), width)
    mix = mixed_depth_pileup(rng, raw.alleles, B, 1.0 if dense else 0.2, quals=quals, dense=dense, deep=0 if dense else 3,
                             doublet_rate=0.0)
    check(m, mix, g, assign, a, make_grid(33))


@pytest.mark.parametrize("n_alt", [3000, 3100])
def test_ambient_deep_pair_at_quality_127(m, n_alt):
    """The rescale's worst case: one pair of ~3 000 reads, every one ALT at quality 127, on a hom-REF row with hard zeros (each read scales
    the cell's term by err(127)/3), at rho = 0 and at the ends of the grid — against ambient_ref, which takes engine.phred_tables()."""
    rng = np.random.default_rng(n_alt)
    S, V = 40, 4
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    g[5, :] = np.array([1.0, 0.0, 0.0], dtype=np.float32)
    deep = np.full(n_alt, (1 << 7) | 127, dtype=np.uint8)
    other = [(s, np.array([(1 << 7) | 127, 127, 0, 1], dtype=np.uint8)) for s in (2, 9, 17)]
    pairs = [other[0], (5, deep)] + other[1:]
    po = np.array([0, len(pairs)], dtype=np.int64)
    ro = np.array([0, sum(len(r) for _, r in pairs)], dtype=np.int64)
    t = np.ones(1, dtype=np.int32)
    sp = m["synth"].SynthPileup(1, S, po, ro, np.array([s for s, _ in pairs], dtype=np.int32), np.array([len(r) for _, r in pairs], dtype=np.uint16),
                                np.concatenate([r for _, r in pairs]).astype(np.uint8), t, t, t, np.array([[0, -1]], dtype=np.int32))
    a = rng.uniform(0.05, 0.95, size=S)
    a[5] = 1.0                                      # the soup is all ALT there: the grid's ends differ by ~90 000 in LL
    grid = np.array([0.0, 1e-12, 1e-6, 0.5, 1.0 - 1e-9, 1.0])
    ll, _, _ = check(m, sp, g, np.zeros(1, dtype=np.int32), a, grid)
    assert np.isfinite(ll).all() and ll[0, 0] < -50000 and ll[0, -1] > -100
