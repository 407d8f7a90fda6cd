"""GPU (-m gpu): the ambient-aware doublet profile (Engine.ambient_doublet_profile / dmx_engine_ambient_doublet, ambient.ambient_calls_run).

LL is checked against the float64 numpy restatement of tests/ambient_dbl_ref.py: |d| <= 1e-9, N.SNP / N.READ exact.  Then the bits
(repeat, rho and alpha grids split, a candidate alone against any slot of C = 8, host against device cand), the symmetry
(v1, v2, alpha) = (v2, v1, 1 - alpha), the tie to k_ambient at alpha = 0, no interference with the engine's other results, argument
errors, two full-size shapes on sampled barcodes, the command line end to end, and the recovery of soupy singlets that the plain pass
calls DBL-."""
import json
import os

import numpy as np
import pytest

import ambient_dbl_ref as D
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
    return np.array([0.15]) if Q == 1 else np.linspace(0.0, 1.0, Q)


def random_cand(rng, B, C, V, unused=0.25):
    v1 = rng.integers(0, V, size=(B, C))
    v2 = (v1 + 1 + rng.integers(0, V - 1, size=(B, C))) % V
    cand = np.stack([v1, v2], axis=2).astype(np.int32)
    cand[rng.random((B, C)) < unused] = -1
    cand[::9] = -1                                   # barcodes with no used slot
    return cand


def run_profile(m, g, pl, cand, alphas, a, grid):
    e = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        out = e.ambient_doublet_profile(cand, alphas, a, grid)
        info = e.ambient_doublet_info()
    finally:
        e.close()
    return out, info


def check(m, sp, g, cand, alphas, a, grid, width=None):
    (ll, n_snp, n_read), info = run_profile(m, g, host_pileup(m, sp, width), cand, alphas, a, grid)
    mat, err = m["engine"].phred_tables()
    LL, ns, nr = D.ref_dbl_profile(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, cand, g, a, alphas, grid, mat, err)
    assert np.array_equal(n_snp, ns) and np.array_equal(n_read, nr)
    d = np.abs(ll - LL).max() if ll.size else 0.0
    print(f"max |LL - restatement| = {d:.3e}")
    assert d <= TOL, d
    assert not ll[cand[:, :, 0] < 0].any() and not n_snp[cand[:, :, 0] < 0].any()
    assert info["n_grid"] == len(grid) and info["n_cells"] == sp.n_cells and info["n_cand"] == cand.shape[1] and info["n_alpha"] == len(alphas)
    assert info["n_used"] == int((cand[:, :, 0] >= 0).sum()) and info["profile_bytes"] == ll.size * 8
    return ll, n_snp, n_read


@pytest.mark.parametrize("B,S,V,delta,rbar,dense,width,C,alphas,Q,soft", [
    (120, 257, 8, 1.0, 1.25, True, 1, 2, (0.0, 0.5, 1.0), 51, False),     # dense
    (100, 257, 2, 1.0, 1.5, True, 4, 1, (0.5,), 65, True),                # dense, u32 read counts, two samples, two grid blocks, soft rows
    (160, 900, 16, 0.05, 2.0, False, 2, 8, (0.0, 0.25, 1.0), 64, True),   # sparse, u16 read counts, eight slots
    (150, 400, 32, 0.3, 1.0, False, 1, 3, (0.3,), 130, False),            # one read per pair: pairs with no stored read; three grid blocks
    (200, 300, 8, 0.002, 1.5, False, 1, 5, (0.1, 0.5, 0.9), 1, False),    # many barcodes have no pair at all; one grid point
])
def test_ambient_dbl_parity(m, B, S, V, delta, rbar, dense, width, C, alphas, Q, soft):
    rng = np.random.default_rng(B * 13 + S + V + Q)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    if soft:
        g = np.stack([m["engine"].geno_from_gp(x, 0.01) for x in m["synth"].raw_gp_from_alleles(rng, raw.alleles)])
    else:
        g = gt_matrix(m, raw)
    g[rng.choice(S, S // 10, replace=False), rng.integers(0, V)] = 0.0               # all-zero rows
    g[rng.choice(S, S // 10, replace=False), 0] = np.array([1.0, 0.0, 0.0], dtype=np.float32)   # rows with hard zeros
    sp, _, _, a = m["synth"].make_ambient_mixed_pileup(rng, raw.alleles, B, delta, rbar, rng.choice([0.0, 0.1, 0.3], size=B),
                                                       rng.random(B) < 0.4, 0.5, dense_layout=dense)
    assert (sp.pair_snp is None) == dense
    a = a.copy()
    a[rng.choice(S, S // 8, replace=False)] = 0.0
    a[rng.choice(S, S // 8, replace=False)] = 1.0
    if delta < 0.01:
        assert (np.diff(sp.cell_pair_off) == 0).sum() > B // 4
    check(m, sp, g, random_cand(rng, B, C, V), np.array(alphas), a, make_grid(Q), width)


def deep_cell(m, rng, S, V):
    """One barcode: a 400-read pair, 90 % ALT at bq 40, on rows that are hom-REF with hard zeros for every sample, between ordinary pairs."""
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    g[5, :] = np.array([1.0, 0.0, 0.0], dtype=np.float32)
    deep = np.where(rng.random(400) < 0.9, (1 << 7) | 40, 35).astype(np.uint8)
    pairs = [(2, np.array([(1 << 7) | 30, 30], dtype=np.uint8)), (5, deep), (9, np.array([40, 40, 40, (1 << 7) | 20, 20, 20, 20, 20, 20], dtype=np.uint8)),
             (17, np.array([(1 << 7) | 127], dtype=np.uint8))]
    po = np.array([0, len(pairs)], dtype=np.int64)
    ro = np.array([0, sum(len(r) for _, r in pairs)], dtype=np.int64)
    t = np.ones(1, dtype=np.int32)
    sp = m["synth"].SynthPileup(1, S, po, ro, np.array([s for s, _ in pairs], dtype=np.int32), np.array([len(r) for _, r in pairs], dtype=np.uint16),
                                np.concatenate([r for _, r in pairs]).astype(np.uint8), t, t, t, np.array([[0, 1]], dtype=np.int32))
    return sp, g


def test_ambient_dbl_deep_pair(m):
    """The hard case of the rescale: the entries that count for a hom-REF x hom-REF candidate are thousands of binades below the largest."""
    rng = np.random.default_rng(19)
    S, V = 40, 4
    sp, g = deep_cell(m, rng, S, V)
    g[5, 3] = np.array([0.0, 0.5, 0.5], dtype=np.float32)       # one sample that does explain ALT reads: a candidate whose entries differ widely
    a = rng.uniform(0.05, 0.95, size=S)
    cand = np.array([[[0, 1], [1, 3], [3, 2], [2, 0]]], dtype=np.int32)
    grid = np.array([0.0, 1e-3, 0.01, 0.2, 0.5, 1.0])
    ll, _, _ = check(m, sp, g, cand, np.array([0.0, 0.3, 0.5, 1.0]), a, grid)
    assert np.isfinite(ll).all() and ll[0, 0, 0, 0] < -2000


@pytest.mark.parametrize("quals", ["full", "edges", "max"])
@pytest.mark.parametrize("dense,width", [(False, 2), (True, 1)])
def test_ambient_dbl_quality_range(m, dense, width, quals):
    """Base qualities 0..127 and the depth mix of tests/quality_mix.py (0..6, 14..17, 40, u16 pairs of 256..300 reads, adversarial pairs)."""
    from quality_mix import mixed_depth_pileup
    rng = np.random.default_rng(6600 + int(dense) + {"full": 0, "edges": 2, "max": 4}[quals])
    S, V, B = (131, 8, 40) if dense else (600, 16, 80)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    a = np.clip(raw.alleles, 0, 1).sum(axis=2).mean(axis=1) / 2.0
    mix = mixed_depth_pileup(rng, raw.alleles, B, 1.0 if dense else 0.2, quals=quals, dense=dense, deep=0 if dense else 3)
    check(m, mix, g, random_cand(rng, B, 2, V), np.array([0.0, 0.5, 1.0]), a, make_grid(17), width)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def test_ambient_dbl_bits(m):
    eng, torch = m["engine"], m["torch"]
    rng = np.random.default_rng(23)
    S, V, B = 700, 8, 180
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    from quality_mix import mixed_depth_pileup
    sp = mixed_depth_pileup(rng, raw.alleles, B, 0.15, quals="edges", deep=2)     # shallow and rescaled pairs
    a = rng.uniform(0.0, 1.0, size=S)
    pl = host_pileup(m, sp)
    cand = random_cand(rng, B, 8, V, unused=0.3)
    alphas = np.array([0.0, 0.2, 0.5, 0.7])
    grid = np.linspace(0.0, 1.0, 100)
    d_cand = torch.from_numpy(cand).to("cuda:0")
    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        r1 = e.ambient_doublet_profile(cand, alphas, a, grid)
        r2 = e.ambient_doublet_profile(cand, alphas, a, grid)
        lo = e.ambient_doublet_profile(cand, alphas, a, grid[:37])
        hi = e.ambient_doublet_profile(cand, alphas, a, grid[37:])
        a_lo = e.ambient_doublet_profile(cand, alphas[:1], a, grid)
        a_hi = e.ambient_doublet_profile(cand, alphas[1:], a, grid)
        dv = e.ambient_doublet_profile(int(d_cand.data_ptr()), alphas, a, grid, n_cand=8)
        assert r1[0].any()
        for x, y in ((r1, r2), (r1, dv)):
            for u, w in zip(x, y):
                assert np.array_equal(bits(u), bits(w))
        assert np.array_equal(bits(r1[0]), bits(np.concatenate([lo[0], hi[0]], axis=3)))
        assert np.array_equal(bits(r1[0]), bits(np.concatenate([a_lo[0], a_hi[0]], axis=2)))
        assert np.array_equal(lo[1], r1[1]) and np.array_equal(a_hi[2], r1[2])
        # a candidate alone (C = 1, 2, 3) against the same candidate in its slot of C = 8, and moved to another slot
        for s in range(8):
            one = e.ambient_doublet_profile(cand[:, s:s + 1], alphas, a, grid)
            assert np.array_equal(bits(one[0][:, 0]), bits(r1[0][:, s])) and np.array_equal(one[1][:, 0], r1[1][:, s])
        for C in (2, 3):
            part = e.ambient_doublet_profile(cand[:, 8 - C:], alphas, a, grid)
            assert np.array_equal(bits(part[0]), bits(r1[0][:, 8 - C:]))
        rev = e.ambient_doublet_profile(cand[:, ::-1], alphas, a, grid)
        assert np.array_equal(bits(rev[0][:, ::-1]), bits(r1[0])) and np.array_equal(rev[2][:, ::-1], r1[2])
        # symmetry: (v1, v2, alpha) = (v2, v1, 1 - alpha), to the tolerance (the nine entries are summed in another order)
        sw = e.ambient_doublet_profile(np.where(cand >= 0, cand[:, :, ::-1], -1), 1.0 - alphas[::-1], a, grid)
        d = np.abs(sw[0][:, :, ::-1, :] - r1[0]).max()
        print(f"symmetry max |d| = {d:.3e}")
        assert d <= TOL
    finally:
        e.close()


def test_ambient_dbl_ties_to_singlet_kernel(m):
    """alpha = 0 with exactly one-hot rows for v2: the doublet profile is the singlet profile of v1 on the same engine."""
    eng = m["engine"]
    rng = np.random.default_rng(27)
    S, V, B = 600, 6, 150
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    g[:, V - 1] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, size=S)]
    sp, _, _, a = m["synth"].make_ambient_mixed_pileup(rng, raw.alleles, B, 0.2, 1.6, rng.choice([0.0, 0.3], size=B), False)
    v1 = (np.arange(B) % (V - 1)).astype(np.int32)
    cand = np.stack([v1, np.full(B, V - 1, dtype=np.int32)], axis=1)[:, None, :]
    grid = m["ambient"].default_grid()
    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(host_pileup(m, sp))
        ll, ns, nr = e.ambient_doublet_profile(cand, [0.0, 0.5], a, grid)
        l1, n1, r1 = e.ambient_profile(v1, a, grid)
    finally:
        e.close()
    assert np.array_equal(ns[:, 0], n1) and np.array_equal(nr[:, 0], r1)
    d = np.abs(ll[:, 0, 0, :] - l1).max()
    print(f"alpha = 0 against k_ambient: max |d| = {d:.3e}")
    assert d <= TOL
    assert np.abs(ll[:, 0, 1, :] - l1).max() > 1.0


def test_ambient_dbl_no_interference(m):
    eng = m["engine"]
    rng = np.random.default_rng(33)
    S, V, B = 700, 8, 200
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp, _, _, a = m["synth"].make_ambient_mixed_pileup(rng, raw.alleles, B, 0.2, 1.4, 0.1, rng.random(B) < 0.3)
    pl = host_pileup(m, sp)
    assign = sp.truth[:, 0].copy()
    grid = m["ambient"].default_grid()
    cand = random_cand(rng, B, 2, V)

    def results(e):
        llks, llk0s = e.get_singlet()
        grid_, l00, summ = e.get_doublet()
        ll = np.zeros((B, len(grid))); n1 = np.zeros(B, dtype=np.int32); n2 = np.zeros(B, dtype=np.int32)
        m["capi"].check(e._L.dmx_engine_get_ambient(e._h, ll.ctypes.data, n1.ctypes.data, n2.ctypes.data))
        return [llks, llk0s, grid_, l00, summ.view(np.uint8), ll, n1, n2]

    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        e.run(); e.sync()
        e.ambient_profile(assign, a, grid)
        base = results(e)
        d0 = e.ambient_doublet_profile(cand, [0.25, 0.5], a, grid)
        after = results(e)
        e.ambient_profile(assign, a, grid)
        d1 = e.ambient_doublet_profile(cand, [0.25, 0.5], a, grid)
        after2 = results(e)
    finally:
        e.close()
    assert base[5].any()
    for other in (after, after2):
        for u, w in zip(base, other):
            assert np.array_equal(bits(u), bits(w))
    for u, w in zip(d0, d1):
        assert np.array_equal(bits(u), bits(w))


def test_ambient_dbl_argument_errors(m):
    capi, eng = m["capi"], m["engine"]
    rng = np.random.default_rng(37)
    S, V, B = 100, 4, 20
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp, _, _, a = m["synth"].make_ambient_mixed_pileup(rng, raw.alleles, B, 0.3, 1.2, 0.1, False)
    ok = np.tile(np.array([[[0, 1]]], dtype=np.int32), (B, 1, 1))
    e = eng.Engine(V, (0.0, 0.5), 0.5)

    def bad(code, cand=ok, alphas=(0.5,), amb=a, grid=(0.0, 0.1)):
        with pytest.raises(capi.DmxError) as ei:
            e.ambient_doublet_profile(cand, alphas, amb, grid)
        assert ei.value.code == code

    try:
        e.set_genotypes(g)
        e.B = B
        bad(-3)                                             # no pileup yet
        e.set_pileup(host_pileup(m, sp))
        with pytest.raises(capi.DmxError) as ei:
            capi.check(e._L.dmx_engine_get_ambient_doublet(e._h, None, None, None))
        assert ei.value.code == -3                          # nothing computed yet
        for g_ in ([], [0.2, 0.1], [0.1, 0.1], [-0.1, 0.2], [0.0, 1.5], list(np.linspace(0, 1, 257))):
            bad(-1, grid=g_)
        for al in ([], [0.5, 0.2], [0.3, 0.3], [-0.1], [1.1], list(np.linspace(0, 1, 9))):
            bad(-1, alphas=al)
        for amb in (np.full(S, 1.2), np.full(S, np.nan), a[:-1]):
            bad(-1, amb=amb)
        for pair in ((0, 0), (0, V), (V, 0), (-2, 1), (1, -1)):
            c = ok.copy(); c[3, 0] = pair
            bad(-1, cand=c)
        bad(-1, cand=np.tile(ok, (1, 9, 1)))                # nine slots
        bad(-1, cand=np.zeros((B, 0, 2), dtype=np.int32))
        with pytest.raises(ValueError):
            e.ambient_doublet_profile(ok[:-1], [0.5], a, [0.0])
        c = ok.copy(); c[5, 0] = (-1, 7)                    # v1 = -1: unused whatever v2 says
        ll, ns, _ = e.ambient_doublet_profile(c, [0.5], a, [0.0, 0.1])
        assert not ll[5].any() and ns[5, 0] == 0 and ll[4].any()
    finally:
        e.close()


@pytest.mark.parametrize("cfg_id", [3, 6])
def test_ambient_dbl_full_size(m, cfg_id):
    """cfg3 (dense, 10k x 50k x 32, GP) and cfg6 (sparse, 20k x 100k x 16): two candidates per barcode, 51 grid points; parity on sampled
    barcodes against numpy over their pairs."""
    torch, eng, A = m["torch"], m["engine"], m["ambient"]
    import bench
    cfg = bench.CONFIGS[cfg_id]
    B, S, V = cfg["B"], cfg["S"], cfg["V"]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0xADB00000 + cfg_id)
    raw, g = bench.genotype_matrix(eng, m["synth"], rng, S, V, cfg["field"])
    dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
    dp = m["st"].make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xADB0 + 1000 * cfg_id, device=dev)
    t0 = dp.truth[:, 0].cpu().numpy().astype(np.int32)
    cand = np.stack([np.stack([t0, (t0 + 1) % V], axis=1), np.stack([(t0 + 2) % V, t0], axis=1)], axis=1).astype(np.int32)
    a = rng.uniform(0.0, 1.0, size=S)
    grid = A.default_grid()
    alphas = np.array([0.5])
    e = eng.Engine(V, cfg["alphas"], 0.5)
    e.set_genotypes(g)
    e.set_pileup_struct(dp.as_struct(), keep=dp)
    ll, n_snp, n_read = e.ambient_doublet_profile(cand, alphas, a, grid)
    info = e.ambient_doublet_info()
    e.close()
    print(f"cfg{cfg_id}: k_ambient_dbl C = 2, A = 1, Q = 51: {info['kernel_ms']:.2f} ms")
    assert info["n_used"] == 2 * B and info["profile_bytes"] == B * 2 * len(grid) * 8
    cells = np.unique(np.concatenate([[0, B - 1], rng.choice(B, 2 if cfg_id == 3 else 12, replace=False)]))
    po = dp.cell_pair_off.cpu().numpy()
    ro = dp.cell_read_off.cpu().numpy()
    mat, err = eng.phred_tables()
    for c in cells:
        p0, p1 = int(po[c]), int(po[c + 1])
        snp = None if dp.pair_snp is None else dp.pair_snp[p0:p1].cpu().numpy()
        nrd = dp.pair_nrd[p0:p1].cpu().numpy()
        reads = dp.reads[int(ro[c]):int(ro[c + 1])].cpu().numpy()
        LL, ns, nr = D.ref_dbl_profile(np.array([0, p1 - p0]), snp, nrd, reads, cand[c:c + 1], g, a, alphas, grid, mat, err)
        assert np.array_equal(ns[0], n_snp[c]) and np.array_equal(nr[0], n_read[c])
        d = np.abs(ll[c] - LL[0]).max()
        assert d <= TOL, (c, d)
    assert n_snp[cells].min() > 0


def test_ambient_dbl_cli_end_to_end(m, tmp_path):
    """--doublets on a small dump: the plain outputs and both ambient files are byte-identical to a run without it, and
    <out>.ambient_calls.tsv has one row per barcode of the .best in byte-wise order, with CALL built from its own columns."""
    A, refine, synth, eng = m["ambient"], m["refine"], m["synth"], m["engine"]
    rng = np.random.default_rng(61)
    S, V, B = 1500, 4, 90
    raw = synth.make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp, _, _, _ = synth.make_ambient_mixed_pileup(rng, raw.alleles, B, 0.2, 1.3, rng.choice([0.0, 0.3], size=B), rng.random(B) < 0.3)
    pl = host_pileup(m, sp)
    samples = [f"S-{j}" for j in range(V)]
    barcodes = [synth.barcode_name(c) for c in range(B)]
    dump = tmp_path / "x.pileup.txt"
    refine.write_pileup_txt(str(dump), refine.PileupDump(samples, [(1, 100 + 10 * j, "A", "C") for j in range(S)], g, barcodes, pl))
    assert A.main(["--pileup", str(dump), "--out", str(tmp_path / "p")]) == 0
    assert not (tmp_path / "p.ambient_calls.tsv").exists()
    assert A.main(["--pileup", str(dump), "--out", str(tmp_path / "d"), "--doublets", "--alpha", "0", "0.25", "0.5"]) == 0
    assert A.main(["--pileup", str(dump), "--out", str(tmp_path / "q"), "--alpha", "0", "0.25", "0.5"]) == 0
    for ext in (".best", ".single", ".sing2", ".ambient.tsv", ".ambient_pool.tsv"):
        assert (tmp_path / ("q" + ext)).read_bytes() == (tmp_path / ("d" + ext)).read_bytes()
    lines = (tmp_path / "d.ambient_calls.tsv").read_text().splitlines()
    assert lines[0] == A.CALLS_HEADER.rstrip("\n")
    best = {t[0]: t[5] for t in (l.split("\t") for l in (tmp_path / "d.best").read_text().splitlines()[1:])}
    rows = [l.split("\t") for l in lines[1:]]
    assert [r[0] for r in rows] == sorted(best, key=str.encode) and all(len(r) == 17 for r in rows)
    kinds = set()
    for r in rows:
        assert r[1] == best[r[0]]
        s1, s2, d, llr = float(r[5]), float(r[8]), float(r[13]), float(r[14])
        assert abs(llr - (d - s1)) < 2e-5 and r[11] in ("0.250", "0.500")
        if abs(d - s1 - 2) > 1e-4 and abs(s1 - s2 - 2) > 1e-4:
            want = f"DBL-{r[9]}-{r[10]}-{r[11]}" if d > s1 + 2 else f"SNG-{r[3]}" if s1 > s2 + 2 else f"AMB-{r[3]}-{r[6]}-{r[9]}/{r[10]}"
            assert r[2] == want
        kinds.add(r[2][:3])
    assert {"SNG", "DBL"} <= kinds
    # --best given: the same calls without the demultiplexing pass
    assert A.main(["--pileup", str(dump), "--out", str(tmp_path / "b2"), "--best", str(tmp_path / "d.best"), "--doublets", "--alpha", "0", "0.25", "0.5"]) == 0
    assert not (tmp_path / "b2.best").exists()
    assert (tmp_path / "b2.ambient_calls.tsv").read_bytes() == (tmp_path / "d.ambient_calls.tsv").read_bytes()


def report(name, **kw):
    d = os.environ.get("DMX_AMBIENT_DBL_REPORT")
    if d:
        with open(d, "a") as f:
            f.write(json.dumps(dict(test=name, **kw)) + "\n")


def test_ambient_dbl_recovery(m, tmp_path):
    """A pool shaped like section 14's recovery fixture (8 donors, 20 000 SNPs, ~2 000 covered SNPs per barcode): singlets at rho 0, 0.2,
    0.4 and 50/50 doublets at rho 0, 0.2, run with --alpha 0 0.1 ... 0.5.  The yardstick is the plain BEST column of the same run.

    Measured on an MI355X (seed 71, 40 barcodes per class): see DESIGN.md section 18."""
    A, synth, eng = m["ambient"], m["synth"], m["engine"]
    rng = np.random.default_rng(71)
    S, V, per = 20000, 8, 40
    raw = synth.make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    classes = [(False, 0.0), (False, 0.2), (False, 0.4), (True, 0.0), (True, 0.2)]
    B = per * len(classes)
    k = np.arange(B) % len(classes)
    dbl = np.array([classes[i][0] for i in k])
    rho = np.array([classes[i][1] for i in k])
    sp, rho, _, _ = synth.make_ambient_mixed_pileup(rng, raw.alleles, B, 0.1, 1.25, rho, dbl, 0.5)
    pl = host_pileup(m, sp)
    samples = [f"S{j}" for j in range(V)]
    barcodes = [synth.barcode_name(c) for c in range(B)]
    alphas = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)
    r = A.ambient_calls_run(pl, g, samples, str(tmp_path / "r"), alphas=alphas, barcodes=barcodes)
    rows, calls = r["rows"], r["calls"]
    assert rows.has_row.all() and 1500 < np.median(r["n_snp"]) < 2500
    call = [A.call_string(c, rows, calls, samples) for c in range(B)]
    t1, t2 = sp.truth[:, 0], sp.truth[:, 1]
    sng_right = lambda names: np.array([names[c] == f"SNG-{samples[t1[c]]}" for c in range(B)])

    def dbl_right(names):
        out = np.zeros(B, dtype=bool)
        for c in np.flatnonzero(dbl):
            p = names[c].split("-")
            out[c] = p[0] == "DBL" and {p[1], p[2]} == {samples[t1[c]], samples[t2[c]]}
        return out

    soupy, clean = ~dbl & (rho >= 0.2), ~dbl & (rho == 0.0)
    best_s, call_s = sng_right(rows.best), sng_right(call)
    best_d, call_d = dbl_right(rows.best), dbl_right(call)
    fig = dict(soupy_best=float(best_s[soupy].mean()), soupy_call=float(call_s[soupy].mean()),
               soupy02_call=float(call_s[~dbl & (rho == 0.2)].mean()), soupy04_call=float(call_s[~dbl & (rho == 0.4)].mean()),
               clean_best=float(best_s[clean].mean()), clean_call=float(call_s[clean].mean()),
               dbl_best=float(best_d[dbl].mean()), dbl_call=float(call_d[dbl].mean()))
    # the restatement's calls on the same inputs
    mat, err = eng.phred_tables()
    csr = (sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads)
    L1, _, _ = R.ref_profile(*csr, rows.sng1, g, r["ambient"], r["grid"], mat, err)
    L2, _, _ = R.ref_profile(*csr, rows.sng2, g, r["ambient"], r["grid"], mat, err)
    LD, _, _ = D.ref_dbl_profile(*csr, r["cand"], g, r["ambient"], r["dbl_alphas"], r["grid"], mat, err)
    ref = A.make_calls(rows, r["cand"], L1, L2, LD, r["dbl_alphas"], r["grid"])
    near = (np.abs(ref.llk_dbl - ref.llk_sng1 - A.CALL_MARGIN) <= 1e-6) | (np.abs(ref.llk_sng1 - ref.llk_sng2 - A.CALL_MARGIN) <= 1e-6)
    fig.update(near_threshold=int(near.sum()), differing_calls=int((ref.call != calls.call).sum()),
               max_abs_diff=float(max(np.abs(LD - r["ll_dbl"]).max(), np.abs(L1 - r["ll_sng1"]).max())))
    print(json.dumps(fig))
    report("recovery", **fig)
    assert r["dbl_alphas"].tolist() == [0.1, 0.2, 0.3, 0.4, 0.5]
    assert fig["soupy_best"] < 0.5, fig                       # the fixture shows the problem
    assert fig["soupy_call"] >= fig["soupy_best"] + 0.5, fig
    assert fig["dbl_call"] >= fig["dbl_best"] - 0.05, fig
    assert fig["clean_call"] >= fig["clean_best"] - 0.02, fig
    assert near.sum() <= 0.01 * B, fig
    assert np.array_equal(ref.call[~near], calls.call[~near]), fig
    assert fig["max_abs_diff"] <= TOL, fig
