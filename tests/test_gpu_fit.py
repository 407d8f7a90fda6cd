"""GPU (-m gpu): the goodness of fit of a call (Engine.fit_profile / dmx_engine_fit, fit.fit_run).

obs / mean / var are checked against the float64 numpy restatement of tests/fit_ref.py: |d| <= tol x max(1, |value|) with
tol = max(1e-9, 100 x drift), drift the float64-against-longdouble difference of the restatement on the same case (measured: 2e-15 to
3e-13 on these pools, so tol = 1e-9; 1.4e-11 on the quality-127 pool, where a pair's variance is a difference of two numbers near 5e4); the four counts exactly.  Then the anchors to the ambient profiles, bit reproducibility, no
interference with the engine's other results, every argument and state error, n_zero, the dropped-donor pool with the CPU test's
assertions, and fit_run end to end.  DMX_ERR_NOMEM is left out: the results take 68 bytes per barcode, so no int32 barcode count exceeds
the free memory of the card."""
import numpy as np
import pytest

import fit_ref as R

pytestmark = pytest.mark.gpu
KEYS = ("obs", "mean", "var", "n_snp", "n_read", "n_trunc", "n_zero")


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import build, capi, engine, fit, refine, synth
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    mat, err = engine.phred_tables()
    return dict(torch=torch, capi=capi, engine=engine, refine=refine, synth=synth, fit=fit, mat=mat, err=err)


def host_pileup(m, sp, width=None):
    nrd = np.asarray(sp.pair_nrd)
    if width is not None:
        nrd = nrd.astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[width])
    return m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, nrd, sp.reads,
                                  sp.rd_totl, sp.rd_pass, sp.rd_uniq)


def gt_matrix(m, raw):
    S = raw.alleles.shape[0]
    return np.stack([m["engine"].geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])


def staged(m, g, pl):
    e = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    e.set_genotypes(g); e.set_pileup(pl)
    return e


def bits(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in KEYS)


def row_bits(r, b):
    return b"".join(np.ascontiguousarray(r[k][b:b + 1]).tobytes() for k in KEYS)


def ref(m, sp, hyp, alpha, rho, a, g, M, mat=None, err=None, **kw):
    return R.ref_fit(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, hyp, alpha, rho, a, g, M, m["mat"] if mat is None else mat,
                     m["err"] if err is None else err, **kw)


def check(m, sp, g, hyp, alpha, rho, a, M, width=None, tables=None):
    e = staged(m, g, host_pileup(m, sp, width))
    try:
        if tables is not None:
            e.set_phred_tables(*tables)
        out = e.fit_profile(hyp, alpha, rho, a, M)
        info = e.fit_info()
    finally:
        e.close()
    kw = {} if tables is None else dict(mat=tables[0], err=tables[1])
    r64 = ref(m, sp, hyp, alpha, rho, a, g, M, **kw)
    rld = ref(m, sp, hyp, alpha, rho, a, g, M, longdouble=True, **kw)
    tol = R.tolerance(r64, rld)
    for k in ("n_snp", "n_read", "n_trunc", "n_zero"):
        assert np.array_equal(out[k], r64[k]), k
    for k in ("obs", "mean", "var"):
        d = R.scaled_difference(out[k], r64[k])
        print(f"{k}: max scaled difference {d:.3g} (tolerance {tol:.3g}, drift {R.drift(r64, rld):.3g})")
        assert d <= tol, (k, d, tol)
    hyp = np.asarray(hyp)
    unused = hyp[:, 0] < 0
    for k in KEYS:
        assert not out[k][unused].any()
    assert info["n_cells"] == sp.n_cells and info["n_used"] == int((~unused).sum()) and info["max_reads"] == M
    assert info["n_singlet"] == int(((hyp[:, 0] >= 0) & (hyp[:, 1] < 0)).sum()) and info["n_doublet"] == int(((hyp[:, 0] >= 0) & (hyp[:, 1] >= 0)).sum())
    assert info["n_trunc"] == int(r64["n_trunc"].sum()) and info["n_zero"] == int(r64["n_zero"].sum())
    return out


def mixed_hypotheses(rng, sp, V):
    """The true calls (singlets and doublets), a fifth of the barcodes unused, a tenth as a wrong singlet; alpha 0, 0.5 or an odd value."""
    B = sp.n_cells
    hyp = sp.truth.copy().astype(np.int32)
    wrong = rng.random(B) < 0.1
    hyp[wrong] = np.stack([rng.integers(0, V, size=int(wrong.sum())), np.full(int(wrong.sum()), -1)], axis=1)
    hyp[rng.random(B) < 0.2] = (-1, -1)
    hyp[0] = (-1, 0)                                                            # v1 = -1: unused whatever v2 says
    alpha = rng.choice([0.0, 0.5, 0.37], size=B)
    return hyp, alpha


@pytest.mark.parametrize("B,S,V,delta,rbar,dense,width,quals,M,soup", [
    (150, 257, 3, 1.0, 1.25, True, 1, None, 1, False),          # dense, M = 1
    (140, 257, 1, 1.0, 3.0, True, 4, "full", 2, True),          # one sample: singlets only; u32 read counts
    (200, 900, 33, 0.05, 3.0, False, 2, "edges", 4, True),      # sparse, u16 read counts, the kept-factor doublet kernel
    (180, 4000, 33, 0.02, 1.25, False, 1, None, 8, False),      # cfg6-like depth at M = 8: the doublet kernel that forms its factors
    (120, 600, 3, 0.2, 3.0, False, 1, "full", 8, True),
    (100, 300, 3, 0.3, 3.0, False, 1, "edges", 3, True),        # M between two instantiations
    (100, 300, 4, 0.3, 3.0, True, 1, None, 5, False),
])
def test_fit_parity(m, B, S, V, delta, rbar, dense, width, quals, M, soup):
    rng = np.random.default_rng(B * 13 + S + V + M)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    g[rng.choice(S, S // 10, replace=False), rng.integers(0, V)] = 0.0               # all-zero rows
    g[rng.choice(S, S // 10, replace=False), 0] = np.array([1.0, 0.0, 0.0], dtype=np.float32)      # rows with hard zeros
    sp = m["synth"].make_pileup(rng, raw.alleles, B, delta, rbar, dense_layout=dense, doublet_rate=0.3, quals=quals)
    assert (sp.pair_snp is None) == (dense and delta >= 1.0)
    hyp, alpha = mixed_hypotheses(rng, sp, V)
    assert V == 1 or ((hyp[:, 1] >= 0) & (hyp[:, 0] >= 0)).sum() > 10
    rho = rng.choice([0.0, 0.1, 0.3], size=B) if soup else None
    a = rng.uniform(0.0, 1.0, size=S) if soup else None
    if soup:
        a[:5] = (0.0, 1.0, 0.0, 1.0, 0.5)
    out = check(m, sp, g, hyp, alpha, rho, a, M, width)
    if rbar >= 3.0 and M < 4:
        assert out["n_trunc"].sum() > 0


def special_pileup(m, cells, S):
    """cells: per barcode a list of (snp, read bytes), SNPs ascending."""
    pairs = [p for c in cells for p in c]
    po = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.int64)
    ro = np.concatenate([[0], np.cumsum([sum(len(r) for _, r in c) for c in cells])]).astype(np.int64)
    t = np.ones(len(cells), dtype=np.int32)
    nrd = np.array([len(r) for _, r in pairs])
    return m["synth"].SynthPileup(len(cells), S, po, ro, np.array([s for s, _ in pairs], dtype=np.int32),
                                  nrd.astype(np.uint16 if nrd.max() > 255 else np.uint8), np.concatenate([r for _, r in pairs]).astype(np.uint8),
                                  t, t, t, np.full((len(cells), 2), -1, dtype=np.int32))


@pytest.mark.parametrize("M", [1, 4, 8])
def test_fit_deep_pair_is_truncated(m, M):
    """One pair of 300 stored reads (u16 counts) among ordinary ones: its first M reads enter, n_trunc counts it."""
    rng = np.random.default_rng(300 + M)
    S, V = 50, 4
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    rd = lambda n: ((rng.integers(0, 2, size=n) << 7) | rng.integers(13, 41, size=n)).astype(np.uint8)
    cells = [[(s, rd(2)) for s in (1, 4, 9)], [(2, rd(1)), (5, rd(300)), (6, rd(9)), (30, rd(3))], [(7, rd(4))]]
    sp = special_pileup(m, cells, S)
    hyp = np.array([[0, -1], [1, 2], [3, -1]], dtype=np.int32)
    out = check(m, sp, g, hyp, np.array([0.0, 0.37, 0.0]), None, None, M)
    assert out["n_trunc"].tolist() == [3 * int(M < 2), 2 + (M < 3), int(M < 4)] and out["n_read"][1] == min(M, 1) + 2 * M + min(M, 3)


def test_fit_quality_127_and_subnormal_weights_need_no_rescaling(m):
    """M = 8, every read at quality 127 and contradicting a hard row whose one entry is a float32 subnormal, for both samples of a doublet:
    the smallest L is (err(127) / 3)^8 times the product of two subnormals, a normal float64; nothing is lost to n_zero."""
    S, V = 12, 3
    sub = np.float32(1e-45)
    assert 0 < sub < np.finfo(np.float32).tiny
    g = np.zeros((S, V, 3), dtype=np.float32)
    g[:, :, 0] = sub                                                            # hom-REF only, subnormal weight
    g[6:, :, :] = np.array([0.25, 0.5, 0.25], dtype=np.float32)
    alt = np.full(8, (1 << 7) | 127, dtype=np.uint8)
    mix = np.array([127, (1 << 7) | 127, 127, 127, (1 << 7) | 127, 127, 127, 127, 127, 127], dtype=np.uint8)
    cells = [[(0, alt), (1, alt[:3]), (7, mix)], [(2, alt), (3, mix), (8, alt)], [(4, alt), (9, mix[:5])]]
    sp = special_pileup(m, cells, S)
    hyp = np.array([[0, 1], [2, -1], [1, 0]], dtype=np.int32)
    out = check(m, sp, g, hyp, np.array([0.5, 0.0, 0.0]), None, None, 8)
    assert out["n_zero"].sum() == 0 and np.isfinite(out["obs"]).all() and out["obs"][0] < -400 and out["n_trunc"].tolist() == [1, 1, 0]
    full = m["synth"].make_pileup(np.random.default_rng(127), np.zeros((S, V, 2), dtype=np.int32) + np.arange(V)[None, :, None] % 2, 40, 0.8, 3.0,
                                  doublet_rate=0.5, quals="max")
    check(m, full, g, full.truth, np.full(40, 0.5), None, None, 8)


def anchor_pool(m, seed, B=160, S=1500, V=6):
    rng = np.random.default_rng(seed)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.1, 1.25, doublet_rate=0.5)
    assert 1 < np.asarray(sp.pair_nrd).max() <= 8                               # nothing is truncated at M = 8
    return rng, sp, g


@pytest.mark.parametrize("rho", [0.0, 0.15])
def test_fit_obs_is_the_ambient_profile(m, rho):
    rng, sp, g = anchor_pool(m, 61)
    B, S = sp.n_cells, sp.n_snps
    a = rng.uniform(0.0, 1.0, size=S)
    assign = sp.truth[:, 0].copy()
    assign[::9] = -1
    hyp = np.stack([assign, np.full(B, -1)], axis=1).astype(np.int32)
    e = staged(m, g, host_pileup(m, sp))
    try:
        out = e.fit_profile(hyp, np.zeros(B), np.full(B, rho), a, 8)
        ll, n_snp, n_read = e.ambient_profile(assign, a, [rho])
    finally:
        e.close()
    assert out["n_trunc"].sum() == 0 and out["n_zero"].sum() == 0
    assert np.array_equal(out["n_snp"], n_snp) and np.array_equal(out["n_read"], n_read)
    assert np.abs(out["obs"] - ll[:, 0]).max() <= 1e-9 and (ll[assign >= 0, 0] < -10).all()


@pytest.mark.parametrize("alpha,rho", [(0.5, 0.0), (0.37, 0.15), (0.0, 0.15)])
def test_fit_obs_is_the_ambient_doublet_profile(m, alpha, rho):
    rng, sp, g = anchor_pool(m, 67)
    B, S = sp.n_cells, sp.n_snps
    a = rng.uniform(0.0, 1.0, size=S)
    hyp = sp.truth.copy().astype(np.int32)
    hyp[hyp[:, 1] < 0] = (-1, -1)
    assert (hyp[:, 0] >= 0).sum() > B // 3
    e = staged(m, g, host_pileup(m, sp))
    try:
        out = e.fit_profile(hyp, np.full(B, alpha), np.full(B, rho), a, 8)
        ll, n_snp, n_read = e.ambient_doublet_profile(hyp[:, None, :], [alpha], a, [rho])
    finally:
        e.close()
    assert out["n_trunc"].sum() == 0 and out["n_zero"].sum() == 0
    assert np.array_equal(out["n_snp"], n_snp[:, 0]) and np.array_equal(out["n_read"], n_read[:, 0])
    assert np.abs(out["obs"] - ll[:, 0, 0, 0]).max() <= 1e-9 and (ll[hyp[:, 0] >= 0, 0, 0, 0] < -10).all()


def permuted(m, sp, perm):
    """The same barcodes in another order: new barcode j is old barcode perm[j]."""
    cell, snp, nrd, start, _ = R.host_pairs(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd)
    po = np.asarray(sp.cell_pair_off)
    cells = []
    for c in perm:
        cells.append([(int(snp[k]), np.asarray(sp.reads)[start[k]:start[k] + nrd[k]]) for k in range(po[c], po[c + 1])])
    return special_pileup(m, cells, sp.n_snps)


def test_fit_bit_reproducibility(m):
    """A barcode's seven outputs depend on its own data, its hypothesis and M only: alone against among others, a repeat, the other
    barcodes in another order, host against device hyp, after an unrelated run() / ambient_profile, on a caller's stream, and rho = None
    against rho = 0."""
    torch = m["torch"]
    rng = np.random.default_rng(71)
    S, V, B, M = 800, 8, 150, 4
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.3, 2.0, doublet_rate=0.4)
    hyp, alpha = mixed_hypotheses(rng, sp, V)
    rho = rng.choice([0.0, 0.2], size=B)
    a = rng.uniform(0.0, 1.0, size=S)
    d_hyp = torch.from_numpy(hyp).to("cuda:0")
    e = staged(m, g, host_pileup(m, sp))
    try:
        r1 = e.fit_profile(hyp, alpha, rho, a, M)
        r2 = e.fit_profile(hyp, alpha, rho, a, M)
        dv = e.fit_profile(int(d_hyp.data_ptr()), alpha, rho, a, M)
        picks = [b for b in (1, 2, 3, 64, B - 1) if hyp[b, 0] >= 0] + [int(np.flatnonzero(hyp[:, 1] >= 0)[0])]
        alone = {}
        for b in picks:
            h = np.full_like(hyp, -1)
            h[b] = hyp[b]
            alone[b] = e.fit_profile(h, alpha, rho, a, M)
        e.run(); e.sync()
        e.ambient_profile(hyp[:, 0], a, [0.0, 0.1])
        r3 = e.fit_profile(hyp, alpha, rho, a, M)
        st = torch.cuda.Stream()
        e.set_stream(st.cuda_stream)
        r4 = e.fit_profile(hyp, alpha, rho, a, M)
        e.set_stream(0)
        z0 = e.fit_profile(hyp, alpha, None, None, M)
        z1 = e.fit_profile(hyp, alpha, np.zeros(B), a, M)
    finally:
        e.close()
    assert r1["n_snp"].sum() > 1000 and r1["var"].any()
    for r in (r2, dv, r3, r4):
        assert bits(r) == bits(r1)
    assert bits(z0) == bits(z1) and bits(z0) != bits(r1)
    for b, r in alone.items():
        assert row_bits(r, b) == row_bits(r1, b) and r["n_snp"].sum() == r1["n_snp"][b]
    perm = rng.permutation(B)
    sp2 = permuted(m, sp, perm)
    e = staged(m, g, host_pileup(m, sp2))
    try:
        rp = e.fit_profile(hyp[perm], alpha[perm], rho[perm], a, M)
    finally:
        e.close()
    for k in KEYS:
        assert rp[k].tobytes() == r1[k][perm].tobytes(), k
    # fewer barcodes: the first 40 alone in a pileup of their own
    sp3 = permuted(m, sp, np.arange(40))
    e = staged(m, g, host_pileup(m, sp3))
    try:
        rs = e.fit_profile(hyp[:40], alpha[:40], rho[:40], a, M)
    finally:
        e.close()
    for k in KEYS:
        assert rs[k].tobytes() == r1[k][:40].tobytes(), k


def test_fit_no_interference(m):
    eng = m["engine"]
    rng = np.random.default_rng(73)
    S, V, B = 700, 8, 200
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp, _, a = m["synth"].make_ambient_pileup(rng, raw.alleles, B, 0.2, 1.4, 0.1)
    pl = host_pileup(m, sp)
    assign = sp.truth[:, 0].copy()
    hyp = np.stack([assign, np.full(B, -1)], axis=1).astype(np.int32)
    hyp[::3, 1] = (hyp[::3, 0] + 1) % V
    cand = hyp[:, None, :].copy()
    cand[hyp[:, 1] < 0] = -1
    grid = [0.0, 0.1, 0.2]

    def results(e):
        llks, llk0s = e.get_singlet()
        grid_, l00, summ = e.get_doublet()
        return [llks, llk0s, grid_, l00, summ.view(np.uint8)]

    x = eng.Engine(V, (0.0, 0.5), 0.5)
    x.set_genotypes(g); x.set_pileup(pl)
    x.run(); x.sync()
    base = results(x)
    amb0 = x.ambient_profile(assign, a, grid)
    dbl0 = x.ambient_doublet_profile(cand, [0.5], a, grid)
    ref0 = x.refine_genotypes(assign, g)
    x.close()
    y = eng.Engine(V, (0.0, 0.5), 0.5)
    y.set_genotypes(g); y.set_pileup(pl)
    f0 = y.fit_profile(hyp, np.full(B, 0.5), np.full(B, 0.1), a, 4)
    y.run(); y.sync()
    amb1 = y.ambient_profile(assign, a, grid)
    dbl1 = y.ambient_doublet_profile(cand, [0.5], a, grid)
    f1 = y.fit_profile(hyp, np.full(B, 0.5), np.full(B, 0.1), a, 4)
    after = results(y)
    ref1 = y.refine_genotypes(assign, g)
    amb2 = [np.zeros_like(amb0[0]), np.zeros_like(amb0[1]), np.zeros_like(amb0[2])]
    m["capi"].check(y._L.dmx_engine_get_ambient(y._h, amb2[0].ctypes.data, amb2[1].ctypes.data, amb2[2].ctypes.data))
    dbl2 = [np.zeros_like(dbl0[0]), np.zeros_like(dbl0[1]), np.zeros_like(dbl0[2])]
    m["capi"].check(y._L.dmx_engine_get_ambient_doublet(y._h, dbl2[0].ctypes.data, dbl2[1].ctypes.data, dbl2[2].ctypes.data))
    f2 = y.fit_profile(hyp, np.full(B, 0.5), np.full(B, 0.1), a, 4)
    y.close()
    for u, w in zip(base, after):
        assert np.array_equal(u.view(np.uint8), w.view(np.uint8))
    for got in (amb1, amb2):
        for u, w in zip(amb0, got):
            assert u.tobytes() == w.tobytes()
    for got in (dbl1, dbl2):
        for u, w in zip(dbl0, got):
            assert u.tobytes() == w.tobytes()
    for u, w in zip(ref0, ref1):
        assert np.array_equal(u.view(np.uint8), w.view(np.uint8))
    assert bits(f0) == bits(f1) == bits(f2) and f0["n_snp"].sum() > 1000


def test_fit_argument_and_state_errors(m):
    capi, eng = m["capi"], m["engine"]
    rng = np.random.default_rng(79)
    S, V, B = 100, 4, 20
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.3, 1.5, doublet_rate=0.0)
    a = rng.uniform(0.0, 1.0, size=S)
    hyp = np.stack([np.arange(B) % V, np.full(B, -1)], axis=1).astype(np.int32)
    al, rho = np.zeros(B), np.full(B, 0.1)

    def fails(e, code, *args, field=None):
        with pytest.raises(capi.DmxError) as ei:
            e.fit_profile(*args)
        assert ei.value.code == code, (ei.value.code, args)
        named(ei, field)

    def named(ei, field=None):                                                  # the message names the entry point and the bad field
        assert "dmx_engine_fit: " in str(ei.value) and (field is None or field in str(ei.value)), (str(ei.value), field)

    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.B, e.S = B, S
        fails(e, capi.DMX_ERR_STATE, hyp, al, rho, a, 4)                        # neither genotypes nor a pileup yet
        e.set_genotypes(g)                                                      # (a pileup cannot be staged before the genotypes)
        fails(e, capi.DMX_ERR_STATE, hyp, al, rho, a, 4)                        # no pileup yet
        e.set_pileup(host_pileup(m, sp))
        for fn, args in (("dmx_engine_get_fit", [None] * 7), ("dmx_engine_fit_info", [C_byref(capi.FitInfo())])):
            with pytest.raises(capi.DmxError) as ei:                           # a query before a call
                capi.check(getattr(e._L, fn)(e._h, *args))
            assert ei.value.code == capi.DMX_ERR_STATE
        for M in (0, 9, -1):
            fails(e, capi.DMX_ERR_ARG, hyp, al, rho, a, M)
        for bad in (-0.1, 1.5, np.nan, np.inf):
            x = al.copy(); x[3] = bad
            fails(e, capi.DMX_ERR_ARG, hyp, x, rho, a, 4, field="alpha[3]")
            x = rho.copy(); x[B - 1] = bad
            fails(e, capi.DMX_ERR_ARG, hyp, al, x, a, 4, field=f"rho[{B - 1}]")
        for bad_a, field in ((np.full(S, 1.2), "ambient[0]"), (np.full(S, np.nan), "ambient[0]"), (a[:-1], "n_snps")):
            fails(e, capi.DMX_ERR_ARG, hyp, al, rho, bad_a, 4, field=field)
        for bad_h in ((V, -1), (-2, -1), (0, V), (1, 1), (0, -2)):
            h = hyp.copy(); h[5] = bad_h
            fails(e, capi.DMX_ERR_ARG, h, al, rho, a, 4, field="hyp[5]")
        fails(e, capi.DMX_ERR_ARG, hyp, al, rho, None, 4, field="rho")          # rho without ambient
        with pytest.raises(ValueError):
            e.fit_profile(hyp[:-1], al, rho, a, 4)
        with pytest.raises(ValueError):
            e.fit_profile(hyp, al[:-1], rho, a, 4)
        rq = capi.FitRequest(B + 1, S, capi.DMX_MEM_HOST, 4, hyp.ctypes.data, al.ctypes.data, None, None)
        for fix in (dict(), dict(n_cells=B, n_snps=S + 1), dict(n_snps=S, hyp_memory=7)):
            for k, v in fix.items():
                setattr(rq, k, v)
            with pytest.raises(capi.DmxError) as ei:
                capi.check(e._L.dmx_engine_fit(e._h, C_byref(rq)))
            assert ei.value.code == capi.DMX_ERR_ARG
            named(ei)
        with pytest.raises(capi.DmxError) as ei:                               # still nothing computed
            capi.check(e._L.dmx_engine_get_fit(e._h, *([None] * 7)))
        assert ei.value.code == capi.DMX_ERR_STATE
        good = e.fit_profile(hyp, al, rho, a, 4)                                # ambient without rho is fine: rho = 0
        zero = e.fit_profile(hyp, al, None, a, 4)
        assert good["n_snp"].sum() > 0 and bits(zero) == bits(e.fit_profile(hyp, al, None, None, 4))
        fails(e, capi.DMX_ERR_ARG, hyp, al, rho, a, 0)
        again = {k: np.zeros_like(good[k]) for k in KEYS}                       # a refused call leaves the last results readable
        capi.check(e._L.dmx_engine_get_fit(e._h, *(again[k].ctypes.data for k in KEYS)))
        assert bits(again) == bits(zero)
        capi.check(e._L.dmx_engine_get_fit(e._h, *([None] * 7)))                # any pointer may be NULL
        e.set_pileup(host_pileup(m, sp))                                        # a new pileup: no result on it yet
        with pytest.raises(capi.DmxError) as ei:
            capi.check(e._L.dmx_engine_get_fit(e._h, *([None] * 7)))
        assert ei.value.code == capi.DMX_ERR_STATE
    finally:
        e.close()


def C_byref(x):
    import ctypes
    return ctypes.byref(x)


def test_fit_zero_likelihood_pairs(m):
    """n_zero: a hard one-hot row contradicted by a quality-0 read, under tables where a quality-0 read cannot be wrong (the engine's own
    tables floor that error, so the engine gets tables of the test's)."""
    S, V = 6, 2
    g = np.zeros((S, V, 3), dtype=np.float32)
    g[:, :, 0] = 1.0                                                            # hom-REF, hard
    mat, err = m["mat"].copy(), m["err"].copy()
    mat[0], err[0] = 1.0, 0.0
    alt0, ref30, alt30 = (1 << 7) | 0, 30, (1 << 7) | 30
    cells = [[(0, np.array([alt0, ref30])), (1, np.array([alt30])), (4, np.array([ref30, alt0, ref30]))],
             [(2, np.array([ref30, ref30])), (3, np.array([ref30, ref30, alt0]))],
             [(5, np.array([alt0]))]]
    sp = special_pileup(m, cells, S)
    hyp = np.array([[0, -1], [0, 1], [1, -1]], dtype=np.int32)
    out = check(m, sp, g, hyp, np.array([0.0, 0.5, 0.0]), None, None, 2, tables=(mat, err))
    assert out["n_zero"].tolist() == [2, 0, 1] and out["n_snp"].tolist() == [1, 2, 0] and out["n_trunc"].tolist() == [0, 1, 0]
    assert out["obs"][2] == 0.0 and out["var"][2] == 0.0 and out["obs"][0] < -5.0


@pytest.fixture(scope="module")
def dropped(m):
    rng = np.random.default_rng(7)
    sp, g, truth = R.dropped_donor_pool(rng, m["synth"], lambda al: m["engine"].geno_from_gt(al, 0.01), 1500, 8, 160, 0.1, 1.25)
    hyp = R.dropped_donor_hypotheses(sp, g, truth, m["mat"], m["err"])
    return sp, g, truth, hyp


def test_fit_dropped_donor_pool(m, dropped):
    """tests/test_fit_cpu.py's pool and assertions, on the engine's numbers."""
    sp, g, truth, hyp = dropped
    out = check(m, sp, g, hyp, np.zeros(sp.n_cells), None, None, 4)
    z = R.zscore(out)
    right, missing = z[truth >= 0], z[truth < 0]
    print(f"power: correct barcodes z {right.min():+.2f} .. {right.max():+.2f}; the dropped donor's cells z <= {missing.max():+.2f}")
    assert len(right) == 140 and len(missing) == 20
    assert (right > -3.0).all(), right.min()
    assert (missing < -4.0).all(), missing.max()


def test_fit_run_end_to_end(m, tmp_path):
    """On a dump of a dropped-donor pool, without --best: .best/.single/.sing2 are byte-identical to a plain run, both files have the
    stated columns, the dropped donor's cells are flagged and fit_donors.tsv counts them.  The pool has twice the SNPs of the one above:
    whatever the plain pass calls a cell of the dropped donor, it misfits (under the restatement its Z is below -29 as any singlet's and
    below -8.8 under every pair of the remaining donors at alpha = 0.5)."""
    F, refine, synth, eng = m["fit"], m["refine"], m["synth"], m["engine"]
    sp, g, truth = R.dropped_donor_pool(np.random.default_rng(7), synth, lambda al: eng.geno_from_gt(al, 0.01), 3000, 8, 160, 0.1, 1.25)
    B, S, V = sp.n_cells, sp.n_snps, g.shape[1]
    pl = host_pileup(m, sp)
    samples = [f"S-{j}" for j in range(V)]
    barcodes = [synth.barcode_name(c) for c in range(B)]
    d = refine.PileupDump(samples, [(1, 100 + 10 * j, "A", "C") for j in range(S)], g, barcodes, pl)
    dump = tmp_path / "x.pileup.txt"
    refine.write_pileup_txt(str(dump), d)
    eng.demuxlet_run(pl, g, samples, (0.0, 0.5), str(tmp_path / "plain"), barcodes=barcodes)
    assert F.main(["--pileup", str(dump), "--out", str(tmp_path / "fit")]) == 0
    for ext in (".best", ".single", ".sing2"):
        assert (tmp_path / ("plain" + ext)).read_bytes() == (tmp_path / ("fit" + ext)).read_bytes()
    rows = [l.split("\t") for l in (tmp_path / "fit.fit.tsv").read_text().splitlines()]
    assert "\t".join(rows[0]) == F.FIT_HEADER.rstrip("\n") and len(rows) == B + 1 and all(len(r) == 14 for r in rows)
    by_bc = {r[0]: r for r in rows[1:]}
    assert [r[0].encode() for r in rows[1:]] == sorted(b.encode() for b in barcodes)
    for c in range(B):
        r = by_bc[barcodes[c]]
        if truth[c] < 0:
            assert r[13] == "MISFIT" and float(r[10]) < -4.0, r
        elif r[1] == f"SNG-S-{truth[c]}":
            assert r[13] == "." and float(r[10]) > -3.0 and r[2] == r[1] and r[12] == r[10], r
    n_right = sum(by_bc[barcodes[c]][1] == f"SNG-S-{truth[c]}" for c in range(B) if truth[c] >= 0)
    assert n_right >= 100
    # Z in the file is the engine's number under the row's hypothesis
    hy = F.read_best_hypotheses(str(tmp_path / "fit.best"), samples, barcodes)
    e = staged(m, g, pl)
    try:
        out = e.fit_profile(hy.hyp, hy.alpha, None, None, 4)
    finally:
        e.close()
    z = R.zscore(out)
    for c in range(B):
        assert by_bc[barcodes[c]][10] == F._num(z[c], ".4f") and int(by_bc[barcodes[c]][3]) == out["n_snp"][c]
    don = [l.split("\t") for l in (tmp_path / "fit.fit_donors.tsv").read_text().splitlines()]
    assert "\t".join(don[0]) == F.DONORS_HEADER.rstrip("\n") and [r[0] for r in don[1:]] == samples + ["DBL", "#POOL"]
    n_flag = sum(r[13] == "MISFIT" for r in rows[1:])
    assert int(don[-1][1]) == B and int(don[-1][4]) == n_flag >= 20
    assert sum(int(r[4]) for r in don[1:-1]) == n_flag and sum(int(r[1]) for r in don[1:-1]) == B
    # --best given: no demultiplexing pass, the same files; --max-reads and --z-min reach the engine and the flags
    assert F.main(["--pileup", str(dump), "--out", str(tmp_path / "b2"), "--best", str(tmp_path / "plain.best")]) == 0
    assert not (tmp_path / "b2.best").exists()
    assert (tmp_path / "b2.fit.tsv").read_bytes() == (tmp_path / "fit.fit.tsv").read_bytes()
    assert (tmp_path / "b2.fit_donors.tsv").read_bytes() == (tmp_path / "fit.fit_donors.tsv").read_bytes()
    assert F.main(["--pileup", str(dump), "--out", str(tmp_path / "b3"), "--best", str(tmp_path / "plain.best"), "--max-reads", "1", "--z-min", "-100"]) == 0
    r3 = [l.split("\t") for l in (tmp_path / "b3.fit.tsv").read_text().splitlines()]
    assert all(r[13] == "." for r in r3[1:]) and all(int(r[4]) == int(r[3]) for r in r3[1:]) and any(int(r[5]) > 0 for r in r3[1:])
    # --ambient-tsv: RHO per barcode from an ambient.py run; a barcode it lists at RHO 0, or does not list, keeps its row to the byte
    from demuxlet_amd import ambient as A
    assert A.main(["--pileup", str(dump), "--out", str(tmp_path / "amb"), "--best", str(tmp_path / "plain.best")]) == 0
    rho = F.read_rho_tsv(str(tmp_path / "amb.ambient.tsv"), barcodes)
    assert (rho > 0).any() and (rho == 0).any()
    assert F.main(["--pileup", str(dump), "--out", str(tmp_path / "b4"), "--best", str(tmp_path / "plain.best"), "--ambient-tsv", str(tmp_path / "amb.ambient.tsv")]) == 0
    r4 = {l.split("\t")[0]: l for l in (tmp_path / "b4.fit.tsv").read_text().splitlines()[1:]}
    r0 = {l.split("\t")[0]: l for l in (tmp_path / "fit.fit.tsv").read_text().splitlines()[1:]}
    same = np.array([r4[barcodes[c]] == r0[barcodes[c]] for c in range(B)])
    assert len(r4) == B and same[rho == 0].all() and (~same[rho > 0]).mean() >= 0.9
