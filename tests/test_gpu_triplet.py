"""GPU (-m gpu): the triplet profile (Engine.triplet_profile / dmx_engine_triplet) and the triplet calls (triplet.triplet_run).

LL is checked against the float64 numpy restatement of tests/triplet_ref.py: |d| <= 1e-9, N.SNP / N.READ exact.  Then the bits (repeat, a
slot alone against any position of C = 8, the share list split, host against device base, other barcodes' slots changed), the ties to
k_ambient_dbl (w3 = 0) and k_ambient (w = (1, 0, 0)) on one-hot columns, the permutation symmetry, no interference with the engine's
other results, argument and state errors, the cfg6 shape on sampled barcodes, the command line end to end, and the recovery of
triplets that the plain pass calls DBL-."""
import json

import numpy as np
import pytest

import ambient_dbl_ref as D
import ambient_ref as R
import triplet_ref as T3

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import ambient, build, capi, cluster, engine, refine, synth, synth_torch, triplet
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return dict(torch=torch, capi=capi, engine=engine, refine=refine, synth=synth, st=synth_torch, ambient=ambient, triplet=triplet, cluster=cluster)


def host_pileup(m, sp, width=None):
    nrd = np.asarray(sp.pair_nrd)
    if width is not None:
        nrd = nrd.astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[width])
    return m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, nrd, sp.reads,
                                  sp.rd_totl, sp.rd_pass, sp.rd_uniq)


def gt_matrix(m, raw):
    S = raw.alleles.shape[0]
    return np.stack([m["engine"].geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])


SHARES8 = np.array([[1 / 3, 1 / 3, 1 / 3], [0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5], [0.7, 0.3, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0],
                    [0.1, 0.2, 0.7]])


def random_base(rng, B, C, V, unused=0.25):
    v1 = rng.integers(0, V, size=(B, C))
    v2 = (v1 + 1 + rng.integers(0, V - 1, size=(B, C))) % V
    base = np.stack([v1, v2], axis=2).astype(np.int32)
    base[rng.random((B, C)) < unused] = -1
    base[::9] = -1                                   # barcodes with no used slot
    return base


def run_profile(m, g, pl, base, shares):
    e = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        out = e.triplet_profile(base, shares)
        info = e.triplet_info()
    finally:
        e.close()
    return out, info


def check(m, sp, g, base, shares, width=None):
    (ll, n_snp, n_read), info = run_profile(m, g, host_pileup(m, sp, width), base, shares)
    mat, err = m["engine"].phred_tables()
    LL, ns, nr = T3.ref_triplet_profile(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, base, g, shares, mat, err)
    assert ll.shape == LL.shape
    assert np.array_equal(n_snp, ns) and np.array_equal(n_read, nr)
    with np.errstate(invalid="ignore"):
        d = np.abs(np.where(ll == LL, 0.0, ll - LL)).max() if ll.size else 0.0        # (-inf on both sides agrees)
    print(f"max |LL - restatement| = {d:.3e}")
    assert d <= TOL, d
    assert not ll[base[:, :, 0] < 0].any() and not n_snp[base[:, :, 0] < 0].any()
    assert info["n_cells"] == sp.n_cells and info["n_base"] == base.shape[1] and info["n_shares"] == len(shares) and info["n_samples"] == g.shape[1]
    assert info["n_used"] == int((base[:, :, 0] >= 0).sum()) and info["profile_bytes"] == ll.size * 8 and info["kernel_ms"] > 0
    return ll, n_snp, n_read


@pytest.mark.parametrize("B,S,V,delta,rbar,dense,width,C,T,soft", [
    (120, 257, 3, 1.0, 1.25, True, 1, 1, 4, False),      # dense, three samples
    (100, 257, 2, 1.0, 1.5, True, 4, 3, 1, True),        # dense, u32 read counts, two samples (every column is v1 or v2), soft rows
    (160, 900, 64, 0.05, 2.0, False, 2, 8, 4, True),     # sparse, u16 read counts, eight slots, one full block of third donors
    (150, 400, 65, 0.3, 1.0, False, 1, 3, 8, False),     # one read per pair: pairs with no stored read; two blocks, eight share triples
    (100, 250, 130, 0.1, 1.5, False, 1, 2, 4, False),    # three blocks: four accumulators per lane
    (200, 300, 8, 0.002, 1.5, False, 1, 3, 4, False),    # many barcodes have no pair at all
])
def test_triplet_parity(m, B, S, V, delta, rbar, dense, width, C, T, soft):
    rng = np.random.default_rng(B * 13 + S + V + T)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    if soft:
        g = np.stack([m["engine"].geno_from_gp(x, 0.01) for x in m["synth"].raw_gp_from_alleles(rng, raw.alleles)])
    else:
        g = gt_matrix(m, raw)
    g[rng.choice(S, S // 10, replace=False), rng.integers(0, V)] = 0.0               # all-zero rows: a base donor for some slots, a third donor for all
    g[rng.choice(S, S // 10, replace=False), 0] = np.array([1.0, 0.0, 0.0], dtype=np.float32)   # rows with hard zeros
    g[rng.choice(S, S // 10, replace=False), V - 1] = np.array([0.0, 0.0, 1.0], dtype=np.float32)
    kinds = np.minimum(1 + np.arange(B) % 3, V)
    sp, _, _ = m["synth"].make_multiplet_pileup(rng, raw.alleles, B, delta, rbar, kinds, (0.5, 0.3, 0.2), dense_layout=dense)
    assert (sp.pair_snp is None) == dense
    if delta < 0.01:
        assert (np.diff(sp.cell_pair_off) == 0).sum() > B // 4
    shares = SHARES8[:T] if T > 1 else SHARES8[7:8]
    check(m, sp, g, random_base(rng, B, C, V), shares, width)


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


def test_triplet_deep_pair(m):
    """The hard case of the rescale: the entries that count for hom-REF donors are thousands of binades below the largest of the 27."""
    rng = np.random.default_rng(19)
    S, V = 40, 5
    sp, g = deep_cell(m, rng, S, V)
    g[5, 3] = np.array([0.0, 0.5, 0.5], dtype=np.float32)       # one sample that does explain ALT reads: as a base donor and as the third
    base = np.array([[[0, 1], [1, 3], [3, 2], [2, 0]]], dtype=np.int32)
    ll, _, _ = check(m, sp, g, base, SHARES8)
    assert np.isfinite(ll).all() and ll[0, 0, 0, 2] < -2000 and ll[0, 0, 0, 3] > ll[0, 0, 0, 2] + 500


@pytest.mark.parametrize("quals", ["full", "edges", "max"])
@pytest.mark.parametrize("dense,width", [(False, 2), (True, 1)])
def test_triplet_quality_range(m, dense, width, quals):
    """Base qualities 0..127 and the depth mix of tests/quality_mix.py (0..6, 14..17, 40, u16 pairs of 256..300 reads, adversarial pairs)."""
    from quality_mix import mixed_depth_pileup
    rng = np.random.default_rng(7700 + int(dense) + {"full": 0, "edges": 2, "max": 4}[quals])
    S, V, B = (131, 8, 40) if dense else (600, 16, 80)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    mix = mixed_depth_pileup(rng, raw.alleles, B, 1.0 if dense else 0.2, quals=quals, dense=dense, deep=0 if dense else 3)
    check(m, mix, g, random_base(rng, B, 2, V), SHARES8[[0, 1, 4, 6]], width)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def test_triplet_bits(m):
    eng, torch = m["engine"], m["torch"]
    rng = np.random.default_rng(23)
    S, V, B = 700, 70, 180
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    from quality_mix import mixed_depth_pileup
    sp = mixed_depth_pileup(rng, raw.alleles, B, 0.15, quals="edges", deep=2)     # shallow and rescaled pairs
    pl = host_pileup(m, sp)
    base = random_base(rng, B, 8, V, unused=0.3)
    d_base = torch.from_numpy(base).to("cuda:0")
    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        r1 = e.triplet_profile(base, SHARES8)
        r2 = e.triplet_profile(base, SHARES8)
        lo = e.triplet_profile(base, SHARES8[:3])
        hi = e.triplet_profile(base, SHARES8[3:])
        dv = e.triplet_profile(int(d_base.data_ptr()), SHARES8, n_base=8)
        assert r1[0].any()
        for x, y in ((r1, r2), (r1, dv)):
            for u, w in zip(x, y):
                assert np.array_equal(bits(u), bits(w))
        assert np.array_equal(bits(r1[0]), bits(np.concatenate([lo[0], hi[0]], axis=2)))
        assert np.array_equal(lo[1], r1[1]) and np.array_equal(hi[2], r1[2])
        # a slot alone (C = 1) against the same slot in its position of C = 8, parts of the list, and the list reversed
        for s in range(8):
            one = e.triplet_profile(base[:, s:s + 1], SHARES8)
            assert np.array_equal(bits(one[0][:, 0]), bits(r1[0][:, s])) and np.array_equal(one[1][:, 0], r1[1][:, s])
        for C in (2, 3):
            part = e.triplet_profile(base[:, 8 - C:], SHARES8)
            assert np.array_equal(bits(part[0]), bits(r1[0][:, 8 - C:]))
        rev = e.triplet_profile(base[:, ::-1], SHARES8[::-1])
        assert np.array_equal(bits(rev[0][:, ::-1, ::-1]), bits(r1[0])) and np.array_equal(rev[2][:, ::-1], r1[2])
        # other barcodes' slots changed: the even barcodes keep theirs
        other = base.copy()
        other[1::2] = random_base(rng, B, 8, V, unused=0.5)[1::2]
        ch = e.triplet_profile(other, SHARES8)
        assert np.array_equal(bits(ch[0][0::2]), bits(r1[0][0::2])) and np.array_equal(ch[1][0::2], r1[1][0::2])
        assert not np.array_equal(ch[0][1::2], r1[0][1::2])
    finally:
        e.close()


def one_hot_pool(m, seed, S, V, B, cols):
    rng = np.random.default_rng(seed)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    for c in cols:
        g[:, c] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, size=S)]
    sp, _, _ = m["synth"].make_multiplet_pileup(rng, raw.alleles, B, 0.2, 1.6, 1 + np.arange(B) % 3, (0.5, 0.3, 0.2))
    return rng, g, sp


def test_triplet_ties_to_the_ambient_kernels(m):
    """On exactly one-hot columns: w3 = 0 is the doublet profile at rho = 0 and alpha = w2; w = (1, 0, 0) is the singlet profile of v1."""
    eng = m["engine"]
    S, V, B = 600, 7, 150
    rng, g, sp = one_hot_pool(m, 27, S, V, B, (V - 2, V - 1))
    v1 = (np.arange(B) % (V - 2)).astype(np.int32)
    v2 = ((v1 + 1 + np.arange(B) % (V - 3)) % (V - 2)).astype(np.int32)
    pair = np.stack([v1, v2], axis=1)[:, None, :]
    hot = np.stack([v1, np.full(B, V - 2, dtype=np.int32)], axis=1)[:, None, :]
    zeros = np.zeros(S)
    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(host_pileup(m, sp))
        lt, nt, rt = e.triplet_profile(pair, [[0.7, 0.3, 0.0], [0.5, 0.5, 0.0], [0.5, 0.25, 0.25]])
        ld, nd, rd = e.ambient_doublet_profile(pair, [0.3, 0.5], zeros, [0.0])
        ls, ns, rs = e.triplet_profile(hot, [[1.0, 0.0, 0.0], [0.5, 0.25, 0.25]])
        l1, n1, r1 = e.ambient_profile(v1, zeros, [0.0])
    finally:
        e.close()
    assert np.array_equal(nt[:, 0, V - 1], nd[:, 0]) and np.array_equal(rt[:, 0, V - 1], rd[:, 0])
    d = np.abs(lt[:, 0, :2, V - 1] - ld[:, 0, :, 0]).max()
    print(f"w3 = 0 against k_ambient_dbl: max |d| = {d:.3e}")
    assert d <= TOL and np.abs(lt[:, 0, 2, V - 1] - ld[:, 0, 1, 0]).max() > 1.0
    assert np.array_equal(ns[:, 0, V - 1], n1) and np.array_equal(rs[:, 0, V - 1], r1)
    d = np.abs(ls[:, 0, 0, V - 1] - l1[:, 0]).max()
    print(f"w = (1, 0, 0) against k_ambient: max |d| = {d:.3e}")
    assert d <= TOL and np.abs(ls[:, 0, 1, V - 1] - l1[:, 0]).max() > 1.0


def test_triplet_permutation_symmetry(m):
    """((a, b), c, (w1, w2, w3)) = ((a, c), b, (w1, w3, w2)) = ((b, a), c, (w2, w1, w3)) on the device, to the tolerance."""
    eng = m["engine"]
    S, V, B = 500, 6, 120
    rng, g, sp = one_hot_pool(m, 29, S, V, B, ())
    a = (np.arange(B) % V).astype(np.int32)
    b = ((a + 1 + np.arange(B) % 2) % V).astype(np.int32)
    c = ((a + 3 + np.arange(B) % 3) % V).astype(np.int32)
    st = lambda x, y: np.stack([x, y], axis=1)[:, None, :]
    w = [0.5, 0.3, 0.2]
    rb = np.arange(B)
    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(host_pileup(m, sp))
        x = e.triplet_profile(st(a, b), [w])[0][rb, 0, 0, c]
        y = e.triplet_profile(st(a, c), [[w[0], w[2], w[1]]])[0][rb, 0, 0, b]
        z = e.triplet_profile(st(b, a), [[w[1], w[0], w[2]]])[0][rb, 0, 0, c]
    finally:
        e.close()
    d = max(np.abs(x - y).max(), np.abs(x - z).max())
    print(f"symmetry max |d| = {d:.3e}")
    assert x.any() and d <= TOL


def test_triplet_no_interference(m):
    """Singlet, doublet, refine, cluster and ambient results are the same bits with and without triplet calls in between, and a triplet
    call between two run() calls changes nothing."""
    eng = m["engine"]
    rng = np.random.default_rng(33)
    S, V, B = 700, 8, 200
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp, _, _ = m["synth"].make_multiplet_pileup(rng, raw.alleles, B, 0.2, 1.4, 1 + np.arange(B) % 3, (0.5, 0.25, 0.25))
    pl = host_pileup(m, sp)
    assign = sp.truth[:, 0].copy()
    a = rng.uniform(0.0, 1.0, size=S)
    grid = m["ambient"].default_grid()
    base = random_base(rng, B, 2, V)
    q = m["cluster"].hwe_prior(np.zeros(S), np.zeros(S))
    prior = np.ascontiguousarray(np.broadcast_to(q[:, None, :], (S, V, 3)))

    def results(e):
        llks, llk0s = e.get_singlet()
        grid_, l00, summ = e.get_doublet()
        ll = np.zeros((B, len(grid))); n1 = np.zeros(B, dtype=np.int32); n2 = np.zeros(B, dtype=np.int32)
        m["capi"].check(e._L.dmx_engine_get_ambient(e._h, ll.ctypes.data, n1.ctypes.data, n2.ctypes.data))
        dl = np.zeros((B, 2, 2, len(grid)))
        m["capi"].check(e._L.dmx_engine_get_ambient_doublet(e._h, dl.ctypes.data, None, None))
        return [llks, llk0s, grid_, l00, summ.view(np.uint8), ll, n1, n2, dl]

    def run(with_trp):
        trp = []
        e = eng.Engine(V, (0.0, 0.5), 0.5)
        try:
            e.set_genotypes(g); e.set_pileup(pl)
            if with_trp:
                trp.append(e.triplet_profile(base, SHARES8[:4]))
            e.cluster_stage()
            e.run_singlet()
            ll, cs = e.cluster_estep(2, 4, np.full((2, 4), -np.log(4)))
            if with_trp:
                trp.append(e.triplet_profile(base, SHARES8[:4]))
            w = e.cluster_weights()
            mst = e.cluster_mstep(None, q)
            ref = e.refine_genotypes(assign, prior, 1e-3)
            e.run(); e.sync()
            e.ambient_profile(assign, a, grid)
            e.ambient_doublet_profile(base, [0.25, 0.5], a, grid)
            first = results(e)
            if with_trp:
                trp.append(e.triplet_profile(base, SHARES8[:4]))
                after = results(e)
                for u, v in zip(first, after):
                    assert np.array_equal(bits(u), bits(v))
            e.run(); e.sync()
            return [*first, *results(e), ll, cs, w, *mst, *ref], trp
        finally:
            e.close()

    (plain, _), (mixed, trp) = run(False), run(True)
    assert len(plain) == len(mixed) and plain[5].any() and plain[8].any()
    for u, v in zip(plain, mixed):
        assert np.array_equal(bits(np.asarray(u)), bits(np.asarray(v)))
    assert trp[0][0].any()
    for other in trp[1:]:
        for u, v in zip(trp[0], other):
            assert np.array_equal(bits(u), bits(v))


def test_triplet_argument_and_state_errors(m):
    capi, eng = m["capi"], m["engine"]
    rng = np.random.default_rng(37)
    S, V, B = 100, 4, 20
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp, _, _ = m["synth"].make_multiplet_pileup(rng, raw.alleles, B, 0.3, 1.2, 3, (0.5, 0.25, 0.25))
    pl = host_pileup(m, sp)
    ok = np.tile(np.array([[[0, 1]]], dtype=np.int32), (B, 1, 1))
    good_shares = [[0.5, 0.25, 0.25]]

    def bad(e, code, base=ok, shares=good_shares):
        with pytest.raises(capi.DmxError) as ei:
            e.triplet_profile(base, shares)
        assert ei.value.code == code

    def good(e):
        ll, ns, _ = e.triplet_profile(ok, good_shares)
        assert ll.shape == (B, 1, 1, V) and ll.any() and ns.any()
        return ll

    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.B, e.S = B, S
        bad(e, capi.DMX_ERR_STATE)                          # neither pileup nor genotypes
        z, zi = np.zeros(3, dtype=np.int64), np.zeros(2, dtype=np.int32)
        e.set_pileup(eng.HostPileup(2, 0, z, z, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), zi, zi, zi))
        bad(e, capi.DMX_ERR_STATE, base=ok[:2])             # a pileup (of no pairs), but no genotypes yet
    finally:
        e.close()
    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g)
        e.B, e.S = B, S
        bad(e, capi.DMX_ERR_STATE)                          # no pileup yet
        e.set_pileup(pl)
        for f in (e._L.dmx_engine_get_triplet,):
            with pytest.raises(capi.DmxError) as ei:
                capi.check(f(e._h, None, None, None))
            assert ei.value.code == capi.DMX_ERR_STATE      # nothing computed yet
        with pytest.raises(capi.DmxError) as ei:
            e.triplet_info()
        assert ei.value.code == capi.DMX_ERR_STATE
        first = good(e)
        for sh in ([[0.5, 0.25, 0.3]], [[0.5, 0.25, 0.25 + 1e-9]], [[1.2, -0.1, -0.1]], [[0.5, 0.6, -0.1]], [[np.nan, 0.5, 0.5]],
                   [[0.5, 0.25, 0.25], [1 / 3, 1 / 3, 1 / 3], [0.5, 0.25, 0.25]], [[0.1 + 0.01 * k, 0.5, 0.4 - 0.01 * k] for k in range(9)],
                   np.zeros((0, 3))):
            bad(e, capi.DMX_ERR_ARG, shares=sh)
            assert np.array_equal(bits(good(e)), bits(first))
        for pair in ((0, 0), (0, V), (V, 0), (-2, 1), (1, -1)):
            c = ok.copy(); c[3, 0] = pair
            bad(e, capi.DMX_ERR_ARG, base=c)
            assert np.array_equal(bits(good(e)), bits(first))
        bad(e, capi.DMX_ERR_ARG, base=np.tile(ok, (1, 9, 1)))       # nine slots
        bad(e, capi.DMX_ERR_ARG, base=np.zeros((B, 0, 2), dtype=np.int32))
        good(e)
        with pytest.raises(ValueError):
            e.triplet_profile(ok[:-1], good_shares)
        with pytest.raises(ValueError):
            e.triplet_profile(ok, [0.5, 0.25, 0.25])
        # counts that do not match the staged pileup / the genotype matrix
        for nb, nsnp in ((B - 1, S), (B, S - 1)):
            sh = np.array(good_shares)
            rq = capi.TripletRequest(nb, capi.DMX_MEM_HOST, ok.ctypes.data, 1, 1, nsnp, 0, sh.ctypes.data)
            with pytest.raises(capi.DmxError) as ei:
                capi.check(e._L.dmx_engine_triplet(e._h, C_byref(rq)))
            assert ei.value.code == capi.DMX_ERR_ARG
        rq = capi.TripletRequest(B, 7, ok.ctypes.data, 1, 1, S, 0, np.array(good_shares).ctypes.data)
        with pytest.raises(capi.DmxError) as ei:
            capi.check(e._L.dmx_engine_triplet(e._h, C_byref(rq)))
        assert ei.value.code == capi.DMX_ERR_ARG            # base_memory
        assert np.array_equal(bits(good(e)), bits(first))
        c = ok.copy(); c[5, 0] = (-1, 7)                    # v1 = -1: unused whatever v2 says
        ll, ns, _ = e.triplet_profile(c, good_shares)
        assert not ll[5].any() and not ns[5].any() and ll[4].any()
    finally:
        e.close()


def test_triplet_widest_pool_and_nomem(m):
    """V = 4 094, the engine's widest pool (16 column blocks): a profile that cannot fit is refused before anything is allocated, and a
    small one on the same engine is right."""
    capi, eng = m["capi"], m["engine"]
    rng = np.random.default_rng(39)
    S, V, B = 6, 4094, 3
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp, _, _ = m["synth"].make_multiplet_pileup(rng, raw.alleles, B, 0.8, 2.0, 3, (0.5, 0.25, 0.25))
    free = m["torch"].cuda.mem_get_info(0)[0]
    nb = int(free // (8 * 8 * V * 8)) + 1024                # barcodes whose 8 x 8 x V profile is larger than the free memory
    po = np.zeros(nb + 1, dtype=np.int64)
    zi = np.zeros(nb, dtype=np.int32)
    base = np.array([[[5, 4000], [-1, -1]], [[4093, 0], [64, 63]], [[255, 256], [3000, 7]]], dtype=np.int32)
    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g)
        e.set_pileup(eng.HostPileup(nb, S, po, po, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), zi, zi, zi))
        with pytest.raises(capi.DmxError) as ei:
            e.triplet_profile(np.full((nb, 8, 2), -1, dtype=np.int32), SHARES8)
        assert ei.value.code == capi.DMX_ERR_NOMEM
        e.set_pileup(host_pileup(m, sp))
        ll, n_snp, n_read = e.triplet_profile(base, SHARES8[:2])
    finally:
        e.close()
    mat, err = eng.phred_tables()
    LL, ns, nr = T3.ref_triplet_profile(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, base, g, SHARES8[:2], mat, err)
    assert np.array_equal(n_snp, ns) and np.array_equal(n_read, nr) and ll[2, 1].all() and not ll[0, 1].any()
    d = np.abs(ll - LL).max()
    print(f"V = 4094: max |LL - restatement| = {d:.3e}")
    assert d <= TOL


def C_byref(x):
    import ctypes
    return ctypes.byref(x)


def test_triplet_full_size(m):
    """cfg6 (sparse, 20k x 100k x 16): two base pairs per barcode, four share triples over all barcodes; parity on 48 sampled barcodes
    against numpy over their pairs."""
    torch, eng = m["torch"], m["engine"]
    import bench
    cfg = bench.CONFIGS[6]
    B, S, V = cfg["B"], cfg["S"], cfg["V"]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0x7B1E0006)
    raw, g = bench.genotype_matrix(eng, m["synth"], rng, S, V, cfg["field"])
    dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
    dp = m["st"].make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0x7B1E + 6000, device=dev)
    t0 = dp.truth[:, 0].cpu().numpy().astype(np.int32)
    base = np.stack([np.stack([t0, (t0 + 1) % V], axis=1), np.stack([(t0 + 2) % V, t0], axis=1)], axis=1).astype(np.int32)
    shares = m["triplet"].default_shares()
    e = eng.Engine(V, cfg["alphas"], 0.5)
    e.set_genotypes(g)
    e.set_pileup_struct(dp.as_struct(), keep=dp)
    ll, n_snp, n_read = e.triplet_profile(base, shares)
    info = e.triplet_info()
    e.close()
    print(f"cfg6: k_triplet C = 2, T = 4, V = {V}: {info['kernel_ms']:.2f} ms")
    assert info["n_used"] == 2 * B and info["profile_bytes"] == B * 2 * 4 * V * 8
    cells = np.unique(np.concatenate([[0, B - 1], rng.choice(B, 46, replace=False)]))
    po = dp.cell_pair_off.cpu().numpy()
    ro = dp.cell_read_off.cpu().numpy()
    mat, err = eng.phred_tables()
    for c in cells:
        p0, p1 = int(po[c]), int(po[c + 1])
        snp = None if dp.pair_snp is None else dp.pair_snp[p0:p1].cpu().numpy()
        nrd = dp.pair_nrd[p0:p1].cpu().numpy()
        reads = dp.reads[int(ro[c]):int(ro[c + 1])].cpu().numpy()
        LL, ns, nr = T3.ref_triplet_profile(np.array([0, p1 - p0]), snp, nrd, reads, base[c:c + 1], g, shares, mat, err)
        assert np.array_equal(ns[0], n_snp[c]) and np.array_equal(nr[0], n_read[c])
        d = np.abs(ll[c] - LL[0]).max()
        assert d <= TOL, (c, d)
    assert n_snp[cells].min() > 0


def multiplet_job(m, rng, S, V, B, delta, rbar, frac_dbl, frac_trp):
    """Singlets, doublets (half 0.5 / 0.5, half 0.7 / 0.3) and triplets (half even thirds, half 0.5 / 0.25 / 0.25), interleaved."""
    synth = m["synth"]
    raw = synth.make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    n_dbl, n_trp = int(round(B * frac_dbl)), int(round(B * frac_trp))
    n_sng = B - n_dbl - n_trp
    kinds = np.concatenate([np.full(n_sng, 1), np.full(n_dbl, 2), np.full(n_trp, 3)])
    half = lambda n: (np.arange(n) % 2 == 1)[:, None]
    shares = np.concatenate([np.tile([[1.0, 0.0, 0.0]], (n_sng, 1)), np.where(half(n_dbl), [[0.7, 0.3, 0.0]], [[0.5, 0.5, 0.0]]),
                             np.where(half(n_trp), [[0.5, 0.25, 0.25]], [[1 / 3, 1 / 3, 1 / 3]])])
    order = rng.permutation(B)
    sp, t3, w = synth.make_multiplet_pileup(rng, raw.alleles, B, delta, rbar, kinds[order], shares[order])
    return g, sp, t3, kinds[order]


def test_triplet_cli_end_to_end(m, tmp_path):
    """A small dump: files written, header, one row per barcode of the .best in byte-wise order, CALL built from its own columns, and
    --best against the built-in first pass gives the same file."""
    T, refine, synth = m["triplet"], m["refine"], m["synth"]
    rng = np.random.default_rng(61)
    S, V, B = 1500, 5, 90
    g, sp, t3, kinds = multiplet_job(m, rng, S, V, B, 0.3, 1.3, 0.3, 0.3)
    pl = host_pileup(m, sp)
    samples = [f"S-{j}" for j in range(V)]
    barcodes = [synth.barcode_name(c) for c in range(B)]
    dump = tmp_path / "x.pileup.txt"
    refine.write_pileup_txt(str(dump), refine.PileupDump(samples, [(1, 100 + 10 * j, "A", "C") for j in range(S)], g, barcodes, pl))
    assert T.main(["--pileup", str(dump), "--out", str(tmp_path / "d")]) == 0
    for ext in (".best", ".single", ".sing2", ".triplet.tsv"):
        assert (tmp_path / ("d" + ext)).exists()
    lines = (tmp_path / "d.triplet.tsv").read_text().splitlines()
    assert lines[0] == T.TRIPLET_HEADER.rstrip("\n")
    best = {t[0]: t[5] for t in (l.split("\t") for l in (tmp_path / "d.best").read_text().splitlines()[1:])}
    rows = [l.split("\t") for l in lines[1:]]
    assert [r[0] for r in rows] == sorted(best, key=str.encode) and all(len(r) == 19 for r in rows) and len(rows) == B
    kinds_seen = set()
    for r in rows:
        assert r[1] == best[r[0]]
        s1, s2, d, t, llr = float(r[4]), float(r[6]), float(r[10]), float(r[15]), float(r[16])
        assert abs(llr - (t - max(d, s1))) < 2e-5 and r[9] == "0.500" and r[13] not in (r[11], r[12])
        if abs(llr - 2) > 1e-4 and abs(d - s1 - 2) > 1e-4 and abs(s1 - s2 - 2) > 1e-4:
            want = f"TRP-{r[11]}-{r[12]}-{r[13]}-{r[14]}" if llr > 2 else f"DBL-{r[7]}-{r[8]}-{r[9]}" if d > s1 + 2 else f"SNG-{r[3]}" if s1 > s2 + 2 \
                else f"AMB-{r[3]}-{r[5]}-{r[7]}/{r[8]}"
            assert r[2] == want
        kinds_seen.add(r[2][:3])
    assert {"SNG", "DBL", "TRP"} <= kinds_seen
    # --best given: the same calls without the demultiplexing pass; explicit shares are taken
    assert T.main(["--pileup", str(dump), "--out", str(tmp_path / "b2"), "--best", str(tmp_path / "d.best")]) == 0
    assert not (tmp_path / "b2.best").exists()
    assert (tmp_path / "b2.triplet.tsv").read_bytes() == (tmp_path / "d.triplet.tsv").read_bytes()
    assert T.main(["--pileup", str(dump), "--out", str(tmp_path / "b3"), "--best", str(tmp_path / "d.best"), "--shares", "0.6,0.2,0.2"]) == 0
    got = {l.split("\t")[14] for l in (tmp_path / "b3.triplet.tsv").read_text().splitlines()[1:]}
    assert got == {"0.600/0.200/0.200"}


def test_triplet_recovery(m, tmp_path):
    """8 donors, ~1 000 covered SNPs per barcode, B = 400: 70 % singlets, 20 % doublets (half 0.7 / 0.3), 10 % triplets (half
    0.5 / 0.25 / 0.25), through triplet_run with its defaults.  No true singlet or doublet is called TRP; at least 0.95 of the true
    triplets are called TRP with exactly their three donors.  The plain `.best` calls the triplets DBL-.

    Measured on an MI355X: see DESIGN.md section 19."""
    T, A, synth, eng = m["triplet"], m["ambient"], m["synth"], m["engine"]
    rng = np.random.default_rng(71)
    S, V, B = 2000, 8, 400
    g, sp, t3, kinds = multiplet_job(m, rng, S, V, B, 0.5, 1.2, 0.2, 0.1)
    assert (kinds == 1).sum() == 280 and (kinds == 2).sum() == 80 and (kinds == 3).sum() == 40
    assert 900 < np.median(np.diff(sp.cell_pair_off)) < 1100
    samples = [f"S{j}" for j in range(V)]
    barcodes = [synth.barcode_name(c) for c in range(B)]
    r = T.triplet_run(host_pileup(m, sp), g, samples, str(tmp_path / "r"), barcodes=barcodes)
    rows, c = r["rows"], r["calls"]
    assert rows.has_row.all() and (tmp_path / "r.triplet.tsv").exists()
    is_trp = c.call == T.CALL_TRP
    named = np.array([{int(c.trp1[k]), int(c.trp2[k]), int(c.trp3[k])} == set(t3[k].tolist()) for k in range(B)])
    plain = [rows.best[k][:3] for k in np.flatnonzero(kinds == 3)]
    fig = dict(trp_among_singlets=int(is_trp[kinds == 1].sum()), trp_among_doublets=int(is_trp[kinds == 2].sum()),
               triplets_right=float((is_trp & named)[kinds == 3].mean()), triplets_called_trp=float(is_trp[kinds == 3].mean()),
               plain_best_of_triplets={k: plain.count(k) for k in sorted(set(plain))},
               singlets_sng=float((c.call[kinds == 1] == A.CALL_SNG).mean()), doublets_dbl=float((c.call[kinds == 2] == A.CALL_DBL).mean()),
               smallest_margin=float(np.abs(c.llr - A.CALL_MARGIN).min()), kernel_ms=r["info"]["kernel_ms"])
    # the restatement on the same inputs
    mat, err = eng.phred_tables()
    LT, _, _ = T3.ref_triplet_profile(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, r["cand"], g, r["shares"], mat, err)
    fig["max_abs_diff"] = float(np.abs(LT - r["ll_trp"]).max())
    print(json.dumps(fig))
    assert fig["trp_among_singlets"] == 0 and fig["trp_among_doublets"] == 0, fig
    assert fig["triplets_right"] >= 0.95, fig
    assert fig["max_abs_diff"] <= TOL, fig
