"""GPU (-m gpu): the site audit (Engine.site_fit / dmx_engine_site_fit, sites.site_run).

The five sums are checked against the float64 numpy restatement of tests/site_ref.py: |d| <= tol x max(1, |value|) with
tol = max(1e-9, 100 x drift), drift the float64-against-longdouble difference of the restatement on the same case; the five counts
exactly.  Every parity shape has a partial last chunk in each list it has (150 singlet + 70 doublet hypotheses: chunks of 64, 64, 22 |
64, 6) and at least three slabs of 512 SNPs with a partial last one.  Then bit equality (a repeat, one chunk per wave, device hyp, a
caller's stream, rho = NULL, after other passes, one SNP alone), the anchor to Engine.fit_profile, no interference with the engine's other
results, every argument and state error, and site_run end to end on the swapped-rows pool with test_site_cpu.py's four conditions.
DMX_ERR_NOMEM is not tested: the partial buffer shrinks to fit its budget and the results take 60 bytes per SNP, so ordinary means do not
exhaust the card."""
import ctypes

import numpy as np
import pytest

import fit_ref as F
import site_ref as R

pytestmark = pytest.mark.gpu
GETTERS = 10


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import build, capi, engine, fit, refine, sites, synth
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    mat, err = engine.phred_tables()
    return dict(torch=torch, capi=capi, engine=engine, refine=refine, synth=synth, fit=fit, sites=sites, mat=mat, err=err)


def host_pileup(m, sp, width=None):
    nrd = np.asarray(sp.pair_nrd)
    if width is not None:
        nrd = nrd.astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[width])
    return m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, nrd, sp.reads,
                                  sp.rd_totl, sp.rd_pass, sp.rd_uniq)


def gt_matrix(m, raw):
    return np.stack([m["engine"].geno_from_gt(raw.alleles[s], 0.01) for s in range(raw.alleles.shape[0])])


def staged(m, g, pl):
    e = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    e.set_genotypes(g); e.set_pileup(pl)
    return e


def bits(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in R.KEYS)


def ref(m, sp, hyp, alpha, rho, a, g, M, mat=None, err=None, **kw):
    return R.ref_site(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, hyp, alpha, rho, a, g, M, m["mat"] if mat is None else mat,
                      m["err"] if err is None else err, **kw)


def compare(m, out, sp, g, hyp, alpha, rho, a, M, **kw):
    r64 = ref(m, sp, hyp, alpha, rho, a, g, M, **kw)
    rld = ref(m, sp, hyp, alpha, rho, a, g, M, longdouble=True, **kw)
    tol = R.tolerance(r64, rld)
    for k in R.COUNTS:
        assert np.array_equal(out[k], r64[k]), k
    for k in R.FLOATS:
        d = R.scaled_difference(out[k], r64[k])
        print(f"{k}: max scaled difference {d:.3g} (tolerance {tol:.3g}, drift {R.drift(r64, rld):.3g})")
        assert d <= tol, (k, d, tol)
    return r64, tol


def check(m, sp, g, hyp, alpha, rho, a, M, width=None, tables=None):
    e = staged(m, g, host_pileup(m, sp, width))
    try:
        if tables is not None:
            e.set_phred_tables(*tables)
        out = e.site_fit(hyp, alpha, rho, a, M)
        info = e.site_fit_info()
    finally:
        e.close()
    r64, _ = compare(m, out, sp, g, hyp, alpha, rho, a, M, **({} if tables is None else dict(mat=tables[0], err=tables[1])))
    sng, dbl = R.listing(hyp)
    assert info["n_cells"] == sp.n_cells and info["n_snps"] == sp.n_snps and info["max_reads"] == M and info["chunk_cells"] == 64
    assert info["n_singlet"] == len(sng) and info["n_doublet"] == len(dbl) and info["n_used"] == len(sng) + len(dbl)
    assert info["n_chunks"] == -(-len(sng) // 64) + -(-len(dbl) // 64) and 1 <= info["n_waves"] <= info["n_chunks"]
    assert info["n_trunc"] == int(r64["n_trunc"].sum()) and info["n_zero"] == int(r64["n_zero"].sum())
    assert info["slab_snps"] > 0 and info["partial_bytes"] >= 64 * sp.n_snps and info["bytes"] > info["partial_bytes"]
    return out, info


def hypotheses(rng, sp, V, n_sng, n_dbl):
    """n_sng singlet and n_dbl doublet hypotheses on randomly chosen barcodes (mostly the truth, a tenth wrong), the rest unused; alpha 0,
    0.5 or an odd value."""
    B = sp.n_cells
    order = rng.permutation(B)
    hyp = np.full((B, 2), -1, dtype=np.int32)
    s, d = order[:n_sng], order[n_sng:n_sng + n_dbl]
    hyp[s, 0] = np.where(rng.random(n_sng) < 0.1, rng.integers(0, V, size=n_sng), sp.truth[s, 0])
    if n_dbl:
        v1 = sp.truth[d, 0]
        v2 = np.where(sp.truth[d, 1] >= 0, sp.truth[d, 1], (v1 + 1 + rng.integers(0, V - 1, size=n_dbl)) % V)
        hyp[d, 0], hyp[d, 1] = v1, v2
        assert (hyp[d, 0] != hyp[d, 1]).all()
    return hyp, rng.choice([0.0, 0.5, 0.37], size=B)


@pytest.mark.parametrize("B,S,V,delta,rbar,dense,width,quals,M,soup,n_sng,n_dbl", [
    (230, 1100, 3, 1.0, 1.25, True, 1, None, 1, False, 150, 70),        # dense: 512 pairs of a barcode inside a slab; M = 1
    (200, 1100, 1, 0.3, 3.0, False, 4, "full", 2, True, 150, 0),        # one sample: singlet hypotheses only; u32 read counts
    (240, 1300, 33, 0.05, 3.0, False, 2, "edges", 4, True, 150, 70),    # u16 read counts, the kept-factor doublet kernel
    (230, 4000, 33, 0.02, 1.25, False, 1, None, 8, False, 150, 70),     # about 10 pairs per (barcode, slab); SNPs nobody covers
    (160, 1100, 3, 0.2, 3.0, False, 1, "full", 8, True, 0, 140),        # doublet hypotheses only (64, 64, 12), factors formed per pattern
    (230, 1100, 3, 0.3, 3.0, False, 1, "edges", 3, True, 150, 70),      # M between two instantiations
    (230, 1100, 4, 0.3, 3.0, True, 1, None, 5, False, 150, 70),
])
def test_site_parity(m, B, S, V, delta, rbar, dense, width, quals, M, soup, n_sng, n_dbl):
    rng = np.random.default_rng(B * 13 + S + V + M)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    g[rng.choice(S, S // 10, replace=False), rng.integers(0, V)] = 0.0               # all-zero rows
    g[rng.choice(S, S // 10, replace=False), 0] = np.array([1.0, 0.0, 0.0], dtype=np.float32)      # rows with hard zeros
    sp = m["synth"].make_pileup(rng, raw.alleles, B, delta, rbar, dense_layout=dense, doublet_rate=0.3 if V > 1 else 0.0, quals=quals)
    assert (sp.pair_snp is None) == (dense and delta >= 1.0)
    hyp, alpha = hypotheses(rng, sp, V, n_sng, n_dbl)
    rho = rng.choice([0.0, 0.1, 0.3], size=B) if soup else None
    a = rng.uniform(0.0, 1.0, size=S) if soup else None
    if soup:
        a[:5] = (0.0, 1.0, 0.0, 1.0, 0.5)
    out, info = check(m, sp, g, hyp, alpha, rho, a, M, width)
    assert -(-S // info["slab_snps"]) >= 3 and S % info["slab_snps"]
    assert out["n_cell"].sum() > 1000 and out["n_alt"].sum() > 0
    if rbar >= 3.0 and M < 4:
        assert out["n_trunc"].sum() > 0
    if delta <= 0.02:
        pairs = np.diff(sp.cell_pair_off).mean() / -(-S // info["slab_snps"])
        assert 5 < pairs < 15 and (out["n_cell"] == 0).any()
    if dense and delta >= 1.0:
        assert info["slab_snps"] > 64


def special_pileup(m, cells, S):
    """cells: per barcode a list of (snp, read bytes), SNPs ascending."""
    pairs = [p for c in cells for p in c]
    po = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.int64)
    ro = np.concatenate([[0], np.cumsum([sum(len(r) for _, r in c) for c in cells])]).astype(np.int64)
    t = np.ones(len(cells), dtype=np.int32)
    nrd = np.array([len(r) for _, r in pairs], dtype=np.int64)
    return m["synth"].SynthPileup(len(cells), S, po, ro, np.array([s for s, _ in pairs], dtype=np.int32),
                                  nrd.astype(np.uint16 if len(nrd) and nrd.max() > 255 else np.uint8),
                                  np.concatenate([r for _, r in pairs]).astype(np.uint8) if pairs else np.zeros(0, dtype=np.uint8),
                                  t, t, t, np.full((len(cells), 2), -1, dtype=np.int32))


def test_site_zero_likelihood_pairs_and_deep_pairs(m):
    """n_zero per SNP: a hard one-hot row contradicted by a quality-0 read, under tables where such a read cannot be wrong; and a pair of 300
    stored reads (u16 counts) whose first M enter."""
    S, V = 6, 2
    g = np.zeros((S, V, 3), dtype=np.float32)
    g[:, :, 0] = 1.0
    mat, err = m["mat"].copy(), m["err"].copy()
    mat[0], err[0] = 1.0, 0.0
    alt0, ref30, alt30 = (1 << 7) | 0, 30, (1 << 7) | 30
    deep = np.where(np.arange(300) % 3 == 0, alt30, ref30)
    cells = [[(0, np.array([alt0, ref30])), (1, np.array([alt30])), (4, np.array([ref30, alt0, ref30]))],
             [(0, np.array([ref30, ref30])), (3, np.array([ref30, ref30, alt0])), (5, deep)],
             [(0, np.array([alt0])), (5, np.array([alt30]))]]
    sp = special_pileup(m, cells, S)
    hyp = np.array([[0, -1], [0, 1], [1, -1]], dtype=np.int32)
    out, _ = check(m, sp, g, hyp, np.array([0.0, 0.5, 0.0]), None, None, 2, tables=(mat, err))
    assert out["n_zero"].tolist() == [2, 0, 0, 0, 1, 0] and out["n_cell"].tolist() == [1, 1, 0, 1, 0, 2]
    assert out["n_trunc"].tolist() == [0, 0, 0, 1, 0, 1] and out["n_read"].tolist() == [2, 1, 0, 2, 0, 3] and out["n_alt"].tolist() == [0, 1, 0, 0, 0, 2]
    assert out["obs"][2] == 0.0 and out["var"][4] == 0.0 and out["exc"][1] > 0.9


def one_snp(m, sp, i):
    """The pileup restricted to the pairs at SNP i: the same barcodes, most of them empty."""
    cell, snp, nrd, start, _ = F.host_pairs(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd)
    cells = [[] for _ in range(sp.n_cells)]
    for k in np.flatnonzero(snp == i):
        cells[cell[k]].append((int(i), np.asarray(sp.reads)[start[k]:start[k] + nrd[k]]))
    return special_pileup(m, cells, sp.n_snps)


def test_site_bit_reproducibility(m):
    """A SNP's ten outputs depend on the pairs at that SNP, their barcodes' hypotheses and list positions and M only: a repeat, one chunk per
    buffer wave against the default budget, host against device hyp, a caller's stream, rho = None against rho = 0, after run(),
    fit_profile and refine_genotypes, and the SNP alone in a pileup of the same barcodes."""
    torch = m["torch"]
    rng = np.random.default_rng(71)
    S, V, B, M = 1100, 8, 240, 4
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.2, 2.0, doublet_rate=0.4)
    hyp, alpha = hypotheses(rng, sp, V, 150, 70)
    rho = rng.choice([0.0, 0.2], size=B)
    a = rng.uniform(0.0, 1.0, size=S)
    d_hyp = torch.from_numpy(hyp).to("cuda:0")
    e = staged(m, g, host_pileup(m, sp))
    try:
        r1 = e.site_fit(hyp, alpha, rho, a, M)
        i1 = e.site_fit_info()
        r2 = e.site_fit(hyp, alpha, rho, a, M)
        rw = e.site_fit(hyp, alpha, rho, a, M, partial_bytes=64 * S)
        iw = e.site_fit_info()
        rw2 = e.site_fit(hyp, alpha, rho, a, M, partial_bytes=2 * 64 * S + 17)
        iw2 = e.site_fit_info()
        dv = e.site_fit(int(d_hyp.data_ptr()), alpha, rho, a, M)
        e.run(); e.sync()
        e.fit_profile(hyp, alpha, rho, a, M)
        e.refine_genotypes(hyp[:, 0], g)
        r3 = e.site_fit(hyp, alpha, rho, a, M)
        st = torch.cuda.Stream()
        e.set_stream(st.cuda_stream)
        r4 = e.site_fit(hyp, alpha, rho, a, M)
        e.set_stream(0)
        z0 = e.site_fit(hyp, alpha, None, None, M)
        z1 = e.site_fit(hyp, alpha, np.zeros(B), a, M)
    finally:
        e.close()
    assert r1["n_cell"].sum() > 10000 and r1["var"].any() and r1["vexc"].any()
    assert i1["n_chunks"] == 5 and i1["n_waves"] == 1 and iw["n_waves"] == 5 and iw["partial_bytes"] == 64 * S and iw2["n_waves"] == 3
    for r in (r2, rw, rw2, dv, r3, r4):
        assert bits(r) == bits(r1)
    assert bits(z0) == bits(z1) and bits(z0) != bits(r1)
    for i in (0, 511, 512, 700, S - 1):
        e = staged(m, g, host_pileup(m, one_snp(m, sp, i)))
        try:
            alone = e.site_fit(hyp, alpha, rho, a, M)
        finally:
            e.close()
        assert r1["n_cell"][i] > 20 and alone["n_cell"].sum() == r1["n_cell"][i]
        for k in R.KEYS:
            assert alone[k][i:i + 1].tobytes() == r1[k][i:i + 1].tobytes(), (i, k)


def test_site_anchor_and_no_interference(m):
    """The sums over the SNPs are Engine.fit_profile's sums over the barcodes; the singlet stage, the grid, the fit results and the refined
    matrix read back unchanged after the call, and a refinement that finds the slab table built by site_fit gives a fresh engine's bits."""
    eng, capi = m["engine"], m["capi"]
    rng = np.random.default_rng(73)
    S, V, B, M = 1100, 8, 230, 4
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp, _, a = m["synth"].make_ambient_pileup(rng, raw.alleles, B, 0.2, 1.4, 0.1)
    pl = host_pileup(m, sp)
    hyp, alpha = hypotheses(rng, sp, V, 150, 70)
    rho = np.full(B, 0.1)
    assign = sp.truth[:, 0].copy()

    def results(e):
        llks, llk0s = e.get_singlet()
        grid_, l00, summ = e.get_doublet()
        fit = {k: np.zeros(B, dtype=np.float64 if k in ("obs", "mean", "var") else np.int32) for k in ("obs", "mean", "var", "n_snp", "n_read", "n_trunc", "n_zero")}
        capi.check(e._L.dmx_engine_get_fit(e._h, *(v.ctypes.data for v in fit.values())))
        ll = np.zeros((S, V, 3)); cnt = [np.zeros((S, V), dtype=np.int32) for _ in range(3)]; gp = np.zeros((S, V, 3), dtype=np.float32)
        capi.check(e._L.dmx_engine_get_refined(e._h, ll.ctypes.data, *(c.ctypes.data for c in cnt), gp.ctypes.data))
        return [llks, llk0s, grid_, l00, summ.view(np.uint8)] + list(fit.values()) + [ll] + cnt + [gp]

    x = staged(m, g, pl)
    try:
        x.run(); x.sync()
        f = x.fit_profile(hyp, alpha, rho, a, M)
        x.refine_genotypes(assign, g)
        before = results(x)
        s = x.site_fit(hyp, alpha, rho, a, M)
        after = results(x)
    finally:
        x.close()
    for u, w in zip(before, after):
        assert np.array_equal(u.view(np.uint8), w.view(np.uint8))
    y = staged(m, g, pl)
    try:
        s0 = y.site_fit(hyp, alpha, rho, a, M)                                   # first on this engine: builds the slab table
        ref1 = y.refine_genotypes(assign, g)
    finally:
        y.close()
    assert bits(s0) == bits(s)
    for u, w in zip(before[-5:], ref1):
        assert np.array_equal(u.view(np.uint8), w.view(np.uint8))
    r64 = ref(m, sp, hyp, alpha, rho, a, g, M)
    tol = R.tolerance(r64, ref(m, sp, hyp, alpha, rho, a, g, M, longdouble=True))
    for k in ("obs", "mean", "var"):
        u, w = float(s[k].sum()), float(f[k].sum())
        print(f"{k}: over SNPs {u!r}, over barcodes {w!r}")
        assert abs(u - w) <= tol * max(1.0, abs(w)), (k, u, w)
    for ks, kf in (("n_cell", "n_snp"), ("n_read", "n_read"), ("n_trunc", "n_trunc"), ("n_zero", "n_zero")):
        assert int(s[ks].sum()) == int(f[kf].sum()) and (ks == "n_zero" or s[ks].sum() > 0)


def test_site_argument_and_state_errors(m):
    capi, eng = m["capi"], m["engine"]
    rng = np.random.default_rng(79)
    S, V, B = 100, 4, 20
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.3, 1.5, doublet_rate=0.0)
    a = rng.uniform(0.0, 1.0, size=S)
    hyp = np.stack([np.arange(B) % V, np.full(B, -1)], axis=1).astype(np.int32)
    al, rho = np.zeros(B), np.full(B, 0.1)

    def fails(e, code, *args, field=None, **kw):
        with pytest.raises(capi.DmxError) as ei:
            e.site_fit(*args, **kw)
        assert ei.value.code == code, (ei.value.code, args)
        named(ei, field)

    def named(ei, field=None):                                                  # the message names the entry point and the bad field
        assert "dmx_engine_site_fit: " in str(ei.value) and (field is None or field in str(ei.value)), (str(ei.value), field)

    def query_fails(e):
        for fn, args in (("dmx_engine_get_site_fit", [None] * GETTERS), ("dmx_engine_site_fit_info", [ctypes.byref(capi.SiteFitInfo())])):
            with pytest.raises(capi.DmxError) as ei:
                capi.check(getattr(e._L, fn)(e._h, *args))
            assert ei.value.code == capi.DMX_ERR_STATE

    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.B, e.S = B, S
        fails(e, capi.DMX_ERR_STATE, hyp, al, rho, a, 4)                        # neither genotypes nor a pileup yet
        e.set_genotypes(g)
        fails(e, capi.DMX_ERR_STATE, hyp, al, rho, a, 4)                        # no pileup yet
        e.set_pileup(host_pileup(m, sp))
        query_fails(e)                                                          # a query before a call
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
        for pb in (64 * S - 1, 1, -1, -64 * S):                                 # a budget below one chunk's worth
            fails(e, capi.DMX_ERR_ARG, hyp, al, rho, a, 4, partial_bytes=pb)
        with pytest.raises(ValueError):
            e.site_fit(hyp[:-1], al, rho, a, 4)
        with pytest.raises(ValueError):
            e.site_fit(hyp, al[:-1], rho, a, 4)
        rq = capi.SiteFitRequest(B + 1, S, capi.DMX_MEM_HOST, 4, hyp.ctypes.data, al.ctypes.data, None, None, 0)
        for fix in (dict(), dict(n_cells=B, n_snps=S + 1), dict(n_snps=S, hyp_memory=7), dict(hyp_memory=capi.DMX_MEM_HOST, hyp=None)):
            for k, v in fix.items():
                setattr(rq, k, v)
            with pytest.raises(capi.DmxError) as ei:
                capi.check(e._L.dmx_engine_site_fit(e._h, ctypes.byref(rq)))
            assert ei.value.code == capi.DMX_ERR_ARG
            named(ei)
        with pytest.raises(capi.DmxError) as ei:
            capi.check(e._L.dmx_engine_site_fit(e._h, None))
        assert ei.value.code == capi.DMX_ERR_ARG
        named(ei)
        query_fails(e)                                                          # still nothing computed
        good = e.site_fit(hyp, al, rho, a, 4, partial_bytes=64 * S)             # exactly one chunk's worth is enough
        zero = e.site_fit(hyp, al, None, a, 4)                                  # ambient without rho is fine: rho = 0
        assert good["n_cell"].sum() > 0 and bits(zero) == bits(e.site_fit(hyp, al, None, None, 4)) and bits(zero) != bits(good)
        fails(e, capi.DMX_ERR_ARG, hyp, al, rho, a, 0)
        again = {k: np.zeros_like(good[k]) for k in R.KEYS}                     # a refused call leaves the last results readable
        capi.check(e._L.dmx_engine_get_site_fit(e._h, *(again[k].ctypes.data for k in R.KEYS)))
        assert bits(again) == bits(zero)
        capi.check(e._L.dmx_engine_get_site_fit(e._h, *([None] * GETTERS)))     # any pointer may be NULL
        none = e.site_fit(np.full_like(hyp, -1), al, rho, a, 4)                 # no used barcode: zero rows
        assert not any(none[k].any() for k in R.KEYS) and e.site_fit_info()["n_chunks"] == 0
        e.set_pileup(host_pileup(m, sp))                                        # a new pileup: no result on it yet
        query_fails(e)
    finally:
        e.close()


def test_site_run_end_to_end(m, tmp_path):
    """site_run over three rounds on the swapped-rows pool (tests/site_ref.swap_pool), with test_site_cpu.py's four conditions on the
    engine's own rounds; round 0's files are byte-identical to a plain run; the tables have the stated columns and the engine's numbers.
    Measured with the restatement and the oracle's BEST calls: see test_site_cpu.py's docstring."""
    sites, refine, synth, eng, fit = m["sites"], m["refine"], m["synth"], m["engine"], m["fit"]
    sp, g, swapped, truth = R.swap_pool(eng, synth)
    B, S, V = sp.n_cells, sp.n_snps, g.shape[1]
    pl = host_pileup(m, sp)
    samples = [f"S-{j}" for j in range(V)]
    barcodes = [synth.barcode_name(c) for c in range(B)]
    snps = [(1, 100 + 10 * j, "A", "C") for j in range(S)]
    eng.demuxlet_run(pl, g, samples, (0.0, 0.5), str(tmp_path / "plain"), barcodes=barcodes)
    out = sites.site_run(pl, g, samples, str(tmp_path / "s"), snps=snps, rounds=3, barcodes=barcodes)
    for ext in (".best", ".single", ".sing2"):
        assert (tmp_path / ("plain" + ext)).read_bytes() == (tmp_path / ("s" + ext)).read_bytes()

    def right(path):
        rows = fit.read_best_hypotheses(path, samples, barcodes)
        return float(np.mean([rows.best[c] == f"SNG-S-{truth[c]}" for c in range(B)]))

    rounds = [(right(str(tmp_path / "s.best")), None, None)]
    for r, k in enumerate(out["rounds"], 1):
        assert k["best"] == str(tmp_path / f"s.r{r}.best") and all((tmp_path / f"s.r{r}{ext}").exists() for ext in (".best", ".single", ".sing2"))
        rounds.append((right(k["best"]), k["flag"], k["site"]["n_cell"]))
        print(f"round {r}: flagged {int(k['flag'].sum())} (clean {int((k['flag'] & ~swapped).sum())}); right singlets {rounds[r - 1][0]:.3f} -> {rounds[r][0]:.3f}; "
              f"kernel {k['info']['kernel_ms']:.3f} ms")
    R.check_swapped_rounds(rounds, swapped, R.SWAP_MIN_CELLS)
    # the tables
    rows = [l.split("\t") for l in (tmp_path / "s.sites.tsv").read_text().splitlines()]
    last = out["rounds"][-1]
    assert "\t".join(rows[0]) == sites.SITES_HEADER.rstrip("\n") and len(rows) == S + 1 and all(len(r) == 18 for r in rows)
    assert [r[:4] for r in rows[1:]] == [[str(x) for x in s] for s in snps]
    assert [r[17] == "MISFIT" for r in rows[1:]] == last["flag"].tolist() and out["n_misfit"] == int(last["flag"].sum())
    z, za = R.zscore(last["site"]), R.zalt(last["site"])
    for i in range(0, S, 7):
        assert rows[i + 1][12] == fit._num(z[i], ".4f") and rows[i + 1][16] == fit._num(za[i], ".4f") and int(rows[i + 1][4]) == last["site"]["n_cell"][i]
    tab = (tmp_path / "s.sites_rounds.tsv").read_text().splitlines()
    assert tab[0] == sites.ROUNDS_HEADER.rstrip("\n") and len(tab) == 4
    f1 = out["rounds"][0]["flag"]
    assert tab[1].split("\t")[:4] == ["1", str(int(f1.sum())), "0", str(int(f1.sum()))] and int(tab[1].split("\t")[4]) > 0
    for r in (2, 3):
        p, q = out["rounds"][r - 2]["flag"], out["rounds"][r - 1]["flag"]
        assert tab[r].split("\t")[:4] == [str(r), str(int(q.sum())), str(int((p & ~q).sum())), str(int((q & ~p).sum()))]
    # the command line on a dump, with --best: one round, the same first audit
    d = refine.PileupDump(samples, snps, g, barcodes, pl)
    refine.write_pileup_txt(str(tmp_path / "x.pileup.txt"), d)
    assert sites.main(["--pileup", str(tmp_path / "x.pileup.txt"), "--out", str(tmp_path / "c"), "--best", str(tmp_path / "plain.best")]) == 0
    assert not (tmp_path / "c.best").exists() and (tmp_path / "c.r1.best").read_bytes() == (tmp_path / "s.r1.best").read_bytes()
    c = [l.split("\t") for l in (tmp_path / "c.sites.tsv").read_text().splitlines()]
    assert [r[17] == "MISFIT" for r in c[1:]] == f1.tolist()
    # --singlets-only: the barcodes that round 0 calls doublets are left out of the audit
    assert sites.main(["--pileup", str(tmp_path / "x.pileup.txt"), "--out", str(tmp_path / "o"), "--best", str(tmp_path / "plain.best"), "--singlets-only",
                       "--max-reads", "1", "--z-min", "-100"]) == 0
    o = [l.split("\t") for l in (tmp_path / "o.sites.tsv").read_text().splitlines()]
    assert sum(int(r[4]) for r in o[1:]) < sum(int(r[4]) for r in c[1:]) and all(r[17] == "." for r in o[1:]) and all(int(r[5]) == int(r[4]) for r in o[1:])
