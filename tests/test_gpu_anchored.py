"""GPU (-m gpu): the anchored doublet search (Engine.doublet_anchored / dmx_engine_doublet_anchored; anchored.anchored_run).

Every evaluated entry is compared bit for bit with the STRICT full grid of Engine.run() on the same data, the anchors and the record with
the numpy restatement of tests/anchored_ref.py on the engine's own grid (indices, llk fields and flags exact; the two printed ratios to
1e-12 relative, test_device_reduce_matches_host_scans' bound), wide panels with the oracle (|d| <= 1e-9, the project's TOL) and with a
scattered V = 8 problem; then the bits (repeat, T, anchor rank, host / device anchors, nrd_width, layout, permutation, a barcode
alone), no interference with the engine's other results, the error codes, the files end to end against the oracle's, the low-depth
pool through --verify, and the command line."""
import numpy as np
import pytest

import anchored_ref as AR
import quality_mix as QM
import unsafe_geno as UG

pytestmark = pytest.mark.gpu
TOL = 1e-9
A2 = (0.0, 0.5)


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import anchored, build, capi, dist, engine, refine, synth
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return dict(torch=torch, capi=capi, engine=engine, refine=refine, synth=synth, anchored=anchored, dist=dist)


def host_pileup(m, sp, width=None):
    nrd = np.asarray(sp.pair_nrd)
    if width is not None:
        nrd = nrd.astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[width])
    return m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, nrd, sp.reads,
                                  sp.rd_totl, sp.rd_pass, sp.rd_uniq)


def run_full(m, pl, g, alphas, mode=None):
    e = m["engine"].Engine(g.shape[1], alphas, 0.5, mode=m["capi"].DMX_MODE_STRICT if mode is None else mode)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        e.run()
        grid, l00, summ = e.get_doublet()
    finally:
        e.close()
    return grid, l00, summ


def run_anch(m, pl, g, alphas, T=2, anchors=None, mode=None):
    e = m["engine"].Engine(g.shape[1], alphas, 0.5, mode=m["capi"].DMX_MODE_STRICT if mode is None else mode)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        e.doublet_anchored(T, anchors)
        res = e.get_anchored()
        res["info"] = e.anchored_info()
    finally:
        e.close()
    return res


def assert_entries(res, grid, l00):
    """c0, pairs and llks00 are the grid's entries, bit for bit; unused slots are 0."""
    assert np.array_equal(res["c0"], grid[:, :, 0, :])
    assert np.array_equal(res["llks00"], l00)
    for b in range(grid.shape[0]):
        assert np.array_equal(res["pairs"][b], AR.pairs_from_grid(grid[b], res["anchors"][b])), b


def assert_records(m, res, grid, l00, alphas, n_pairs, anchors=None):
    """Anchors and records equal the restatement's on the engine's own grid."""
    T = res["anchors"].shape[1]
    dt = m["capi"].SUMMARY_DTYPE
    for b in range(grid.shape[0]):
        anc, s = AR.record(grid[b], l00[b], alphas, 0.5, int(n_pairs[b]), dt, anchors=None if anchors is None else anchors[b], T=T)
        assert np.array_equal(res["anchors"][b], anc), (b, res["anchors"][b], anc)
        r = res["summary"][b]
        for f in AR.INDEX_FIELDS + AR.LLK_FIELDS + ("flags",):
            assert r[f] == s[f], (b, f, r[f], s[f])
        if n_pairs[b] > 0:
            assert r["max_llk"] == s["max_llk"], b
        for x, y in zip(AR.ratios(r), AR.ratios(s)):
            assert abs(x - y) <= 1e-12 * abs(y), (b, x, y)
        for f in ("llk_ab", "llk_ba", "llk_ab_alt", "llk_ba_alt", "ev_x_ab", "ev_t_ab", "ev_x_ba", "ev_t_ba"):
            assert r[f] == 0.0


def problem(m, seed, B, S, V, delta, rbar, dense=False, field="GT"):
    rng = np.random.default_rng(seed)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, delta, rbar, dense_layout=dense, doublet_rate=0.3)
    g = QM.genotypes(m["engine"], rng, raw.alleles, field)
    return sp, g


SHAPES = [
    # B, S, V, alphas, delta, rbar, dense, width, Ts, field
    (100, 300, 2, A2, 1.0, 1.5, True, 4, (1, 2), "GT"),
    (120, 257, 3, A2, 1.0, 1.25, True, 1, (3,), "GT"),
    (203, 900, 16, A2, 0.05, 2.0, False, 2, (2,), "GT"),        # a barcode count that is no multiple of 4
    (203, 900, 16, A2, 0.05, 2.0, False, 2, (2,), "GP"),
    (203, 900, 16, A2, 0.05, 2.0, False, 2, (2,), "PL"),
    (61, 400, 33, (0.0, 0.3, 0.5), 0.3, 1.25, False, 1, (4,), "GT"),
    (61, 400, 33, (0.0, 0.3, 0.5), 0.3, 1.25, False, 1, (4,), "GP"),
    (61, 400, 33, (0.0, 0.3, 0.5), 0.3, 1.25, False, 1, (4,), "PL"),
    (40, 300, 64, A2, 0.3, 1.0, False, 1, (2,), "GT"),
    (40, 300, 65, A2, 0.3, 1.0, False, 1, (2,), "GT"),
    (12, 250, 130, A2, 0.1, 1.5, False, 1, (8,), "GT"),
    (9, 150, 70, (0.0, 0.1, 0.25, 0.4, 0.5), 0.3, 1.5, False, 1, (3,), "GT"),
    (200, 300, 8, A2, 0.002, 1.5, False, 1, (2,), "GT"),        # most barcodes have no pair
    (30, 200, 12, (0.1, 0.5), 0.3, 1.25, False, 1, (2,), "GT"), # alpha[0] != 0
    (24, 120, 16, A2, 1.0, 20.0, True, 2, (2,), "GT"),          # pairs deeper than 15 reads
]


@pytest.mark.parametrize("B,S,V,alphas,delta,rbar,dense,width,Ts,field", SHAPES)
def test_entries_are_the_full_grids_bits(m, B, S, V, alphas, delta, rbar, dense, width, Ts, field):
    sp, g = problem(m, 7000 + B + S + V, B, S, V, delta, rbar, dense, field)
    assert (sp.pair_snp is None) == dense
    n_pairs = np.diff(sp.cell_pair_off)
    if delta < 0.01:
        assert (n_pairs == 0).sum() > B // 4
    if rbar > 15:
        assert sp.pair_nrd.max() > 15
    pl = host_pileup(m, sp, width)
    grid, l00, _ = run_full(m, pl, g, alphas)
    for T in Ts:
        res = run_anch(m, pl, g, alphas, T)
        assert_entries(res, grid, l00)
        assert_records(m, res, grid, l00, alphas, n_pairs)
        inf = res["info"]
        assert (inf["n_cells"], inf["n_samples"], inf["n_alpha"], inf["n_anchor"]) == (B, V, len(alphas), T)
        assert inf["n_entries"] == int(m["anchored"].entries_per_barcode(res["anchors"], V, len(alphas)).sum())
        assert inf["result_bytes"] >= res["c0"].nbytes + res["pairs"].nbytes and inf["col_ms"] > 0 and inf["pair_ms"] > 0 and inf["reduce_ms"] > 0


def test_every_base_quality_and_depth(m):
    """A quality_mix pileup: base qualities 0 .. 127, depths 0 .. 40 and a few pairs of hundreds of reads."""
    rng = np.random.default_rng(77)
    raw = m["synth"].make_raw_genotypes(rng, 200, 16)
    sp = QM.mixed_depth_pileup(rng, raw.alleles, 48, 0.3, quals="full", deep=3)
    assert (sp.reads & 127).min() == 0 and (sp.reads & 127).max() == 127
    g = QM.genotypes(m["engine"], rng, raw.alleles, "GT")
    pl = host_pileup(m, sp)
    grid, l00, _ = run_full(m, pl, g, A2)
    res = run_anch(m, pl, g, A2, 2)
    assert_entries(res, grid, l00)
    assert_records(m, res, grid, l00, A2, np.diff(sp.cell_pair_off))


@pytest.mark.parametrize("B,S,V,full", [(4, 200, 100, True), (2, 60, 600, False)])
def test_wide_panels_against_the_oracle(m, oracle, B, S, V, full):
    """|d| <= 1e-9 on every evaluated entry; the V = 600 case never allocates the full grid on the device."""
    rng = np.random.default_rng(1000 + B + V)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.3 if V == 100 else 0.4, 1.25, doublet_rate=0.3)
    g = np.stack([oracle.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    ref = QM.oracle_run(oracle, sp, g)
    res = run_anch(m, host_pileup(m, sp), g, A2, 2)
    d = [np.abs(res["c0"] - ref.llksAB[:, :, 0, :]).max(), np.abs(res["llks00"] - ref.llks00).max()]
    for b in range(B):
        d.append(np.abs(res["pairs"][b] - AR.pairs_from_grid(ref.llksAB[b], res["anchors"][b])).max())
    print(f"V={V}: max|d| = {max(d):.3e}")
    assert max(d) <= TOL
    if full:
        grid, l00, _ = run_full(m, host_pileup(m, sp), g, A2)
        assert_entries(res, grid, l00)


@pytest.mark.parametrize("V,alphas", [(4, A2), (8, (0.0, 0.25, 0.5))])
def test_with_every_sample_an_anchor_the_record_is_k3s(m, V, alphas):
    sp, g = problem(m, 4242 + V, 90, 400, V, 0.2, 1.5)
    pl = host_pileup(m, sp)
    grid, l00, summ = run_full(m, pl, g, alphas)
    res = run_anch(m, pl, g, alphas, V)
    assert_entries(res, grid, l00)
    n_pairs = np.diff(sp.cell_pair_off)
    assert_records(m, res, grid, l00, alphas, n_pairs)
    for b in range(sp.n_cells):
        for f in AR.INDEX_FIELDS + AR.LLK_FIELDS:
            assert res["summary"][b][f] == summ[b][f], (b, f)


def test_a_wide_panel_gives_the_bits_of_the_small_problem(m):
    """A V = 8 problem scattered into columns of a V = 1024 matrix (sample 0 stays 0, the other rows random), explicit anchors at the
    mapped ids: the entries at the mapped partners are the V = 8 run's, and no V x V grid is ever made."""
    cols = np.array([0, 5, 63, 64, 700, 701, 1022, 1023])
    sp, g8 = problem(m, 99, 25, 300, 8, 0.2, 1.5)
    rng = np.random.default_rng(5)
    S = g8.shape[0]
    raw = m["synth"].make_raw_genotypes(rng, S, 1024)
    g = QM.genotypes(m["engine"], rng, raw.alleles, "GT")
    g[:, cols] = g8
    pl = host_pileup(m, sp)
    small = run_anch(m, pl, g8, A2, 3)
    anc = np.where(small["anchors"] >= 0, cols[np.maximum(small["anchors"], 0)], -1).astype(np.int32)
    wide = run_anch(m, pl, g, A2, anchors=anc)
    assert np.array_equal(wide["anchors"], anc)
    assert np.array_equal(wide["c0"][:, cols], small["c0"])
    assert np.array_equal(wide["pairs"][:, :, cols], small["pairs"])          # (llks00 weighs by gp0s, the mean over ALL samples: the panel's own)
    assert wide["info"]["result_bytes"] < 25 * 1024 * 1024 * 2 * 8 // 50


def test_bits_do_not_depend_on_how_the_call_is_made(m):
    sp, g = problem(m, 31337, 70, 500, 20, 0.15, 1.6)
    V, B = 20, sp.n_cells
    pl = host_pileup(m, sp)
    base = run_anch(m, pl, g, A2, 4)
    again = run_anch(m, pl, g, A2, 4)
    for k in ("anchors", "c0", "pairs", "llks00"):
        assert np.array_equal(base[k], again[k]), k
    assert base["summary"].tobytes() == again["summary"].tobytes()
    grid = np.full((B, V, V, 2), np.nan)                      # every entry seen so far, by (j, k, n)

    def fold(res):
        """Every entry of a result agrees with what any earlier call gave for the same (b, j, k, n)."""
        for b in range(B):
            for t, a in enumerate(res["anchors"][b]):
                if a < 0:
                    continue
                for o, view in ((0, grid[b, a, :, 1:]), (1, grid[b, :, a, 1:])):
                    new = res["pairs"][b, t, :, o, :]
                    keep = np.arange(V) != a
                    seen = ~np.isnan(view[keep])
                    assert np.array_equal(view[keep][seen], new[keep][seen]), (b, t, o)
                    view[keep] = new[keep]
    fold(base)
    # T = 1 and 8, the anchors reversed (another rank), an entry reached through two anchors: one value each
    for T in (1, 8):
        r = run_anch(m, pl, g, A2, T)
        assert np.array_equal(r["c0"], base["c0"]) and np.array_equal(r["anchors"][:, :min(T, 4)], base["anchors"][:, :min(T, 4)])
        fold(r)
    rev = np.ascontiguousarray(base["anchors"][:, ::-1])
    r = run_anch(m, pl, g, A2, anchors=rev)
    fold(r)
    assert np.array_equal(r["pairs"], base["pairs"][:, ::-1])
    for f in AR.INDEX_FIELDS + AR.LLK_FIELDS + ("max_llk", "flags"):
        assert np.array_equal(r["summary"][f], base["summary"][f]), f
    # host against device anchors
    d_anc = m["torch"].from_numpy(rev).cuda()
    e = m["engine"].Engine(V, A2, 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        e.doublet_anchored(4, int(d_anc.data_ptr()))
        dev = e.get_anchored()
    finally:
        e.close()
    for k in ("anchors", "c0", "pairs", "llks00"):
        assert np.array_equal(dev[k], r[k]), k
    assert dev["summary"].tobytes() == r["summary"].tobytes()
    # nrd_width 1 / 2 / 4
    for w in (1, 2, 4):
        x = run_anch(m, host_pileup(m, sp, w), g, A2, 4)
        assert np.array_equal(x["pairs"], base["pairs"]) and np.array_equal(x["c0"], base["c0"]) and x["summary"].tobytes() == base["summary"].tobytes()
    # a permutation of the cells permutes the results; a barcode alone gives its own bits
    perm = np.random.default_rng(1).permutation(B)
    x = run_anch(m, m["dist"].slice_pileup(pl, perm), g, A2, 4)
    for k in ("anchors", "c0", "pairs", "llks00"):
        assert np.array_equal(x[k], base[k][perm]), k
    assert x["summary"].tobytes() == base["summary"][perm].tobytes()
    b = int(np.argmax(np.diff(sp.cell_pair_off)))
    x = run_anch(m, m["dist"].slice_pileup(pl, np.array([b])), g, A2, 4)
    for k in ("anchors", "c0", "pairs", "llks00"):
        assert np.array_equal(x[k][0], base[k][b]), k


def test_dense_and_sparse_layouts_of_one_pileup(m):
    sp, g = problem(m, 555, 50, 130, 10, 1.0, 1.4, dense=True)
    assert sp.pair_snp is None
    import dataclasses
    sparse = dataclasses.replace(sp, pair_snp=np.tile(np.arange(sp.n_snps, dtype=np.int32), sp.n_cells))
    a, b = run_anch(m, host_pileup(m, sp), g, A2, 3), run_anch(m, host_pileup(m, sparse), g, A2, 3)
    for k in ("anchors", "c0", "pairs", "llks00"):
        assert np.array_equal(a[k], b[k]), k
    assert a["summary"].tobytes() == b["summary"].tobytes()


def test_the_engines_other_results_stay(m):
    """run() results, get_doublet and an ambient profile are the same before and after; a FAST engine gives the STRICT anchored bits."""
    sp, g = problem(m, 808, 60, 400, 12, 0.2, 1.5)
    pl = host_pileup(m, sp)
    e = m["engine"].Engine(12, A2, 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        e.run()
        before = (e.get_singlet(), e.get_doublet(), e.get_sing())
        asg = (np.arange(sp.n_cells) % 12).astype(np.int32)
        amb0 = e.ambient_profile(asg, np.full(sp.n_snps, 0.3), np.array([0.0, 0.1]))
        e.doublet_anchored(3)
        res = e.get_anchored()
        after = (e.get_singlet(), e.get_doublet(), e.get_sing())
        amb1 = e.ambient_profile(asg, np.full(sp.n_snps, 0.3), np.array([0.0, 0.1]))
    finally:
        e.close()
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0]))
    assert np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1]) and before[1][2].tobytes() == after[1][2].tobytes()
    assert np.array_equal(before[2], after[2])
    assert all(np.array_equal(x, y) for x, y in zip(amb0, amb1))
    assert_entries(res, before[1][0], before[1][1])
    fast = run_anch(m, pl, g, A2, 3, mode=m["capi"].DMX_MODE_FAST)
    for k in ("anchors", "c0", "pairs", "llks00"):
        assert np.array_equal(fast[k], res[k]), k
    assert fast["summary"].tobytes() == res["summary"].tobytes()


def test_errors(m):
    capi, E = m["capi"], m["engine"]
    sp, g = problem(m, 11, 20, 200, 6, 0.3, 1.5)
    pl = host_pileup(m, sp)

    def code(fn):
        with pytest.raises(capi.DmxError) as ex:
            fn()
        return ex.value.code, str(ex.value)

    e = E.Engine(6, A2, 0.5)
    try:
        assert code(lambda: e.get_anchored())[0] == capi.DMX_ERR_STATE
        assert code(lambda: e.anchored_info())[0] == capi.DMX_ERR_STATE
        assert code(lambda: e.doublet_anchored(2))[0] == capi.DMX_ERR_STATE          # neither pileup nor genotypes
        e.set_genotypes(g)
        assert code(lambda: e.doublet_anchored(2))[0] == capi.DMX_ERR_STATE          # genotypes, still no pileup
        e.set_pileup(pl)
        for T in (0, 7, 9):
            assert code(lambda: e.doublet_anchored(T))[0] == capi.DMX_ERR_ARG
        bad = np.tile(np.array([[0, 1]], dtype=np.int32), (20, 1))
        for a, b in ((6, 1), (-2, 1), (3, 3)):
            x = bad.copy(); x[7] = (a, b)
            assert code(lambda: e.doublet_anchored(anchors=x))[0] == capi.DMX_ERR_ARG
        x = bad.copy(); x[7] = (-1, -1)
        e.doublet_anchored(anchors=x)                                                # unused slots are fine
        r = e.get_anchored()
        assert not r["pairs"][7].any() and r["pairs"][6].any()
        rq = capi.AnchoredRequest(19, 2, capi.DMX_MEM_HOST, 0, None)
        import ctypes
        assert e._L.dmx_engine_doublet_anchored(e._h, ctypes.byref(rq)) == capi.DMX_ERR_ARG      # n_cells
        e.get_anchored()                                                             # the last good result is still there
    finally:
        e.close()
    e = E.Engine(6, (0.5,), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        assert code(lambda: e.doublet_anchored(2))[0] == capi.DMX_ERR_ARG            # A < 2
    finally:
        e.close()
    e = E.Engine(1, A2, 0.5)
    try:
        e.set_genotypes(np.ascontiguousarray(g[:, :1])); e.set_pileup(pl)
        assert code(lambda: e.doublet_anchored(1))[0] == capi.DMX_ERR_ARG            # V < 2
    finally:
        e.close()
    # an unsafe matrix is refused, and the message names the full grid
    spu, gu = problem(m, 12, 8, 300, 6, 0.5, 1.5)
    poisoned, _ = UG.poison(gu, "zero", np.random.default_rng(0), spu)
    assert not UG.is_safe(poisoned)
    e = E.Engine(6, A2, 0.5)
    try:
        e.set_genotypes(poisoned); e.set_pileup(host_pileup(m, spu))
        c, msg = code(lambda: e.doublet_anchored(2))
        assert c == capi.DMX_ERR_ARG and "full grid" in msg
    finally:
        e.close()


def test_the_forced_check_switch_does_not_refuse_a_safe_matrix(m, monkeypatch):
    """DMX_FORCE_CHECK makes the full grid's kernels keep their argument test; the anchored pass has no such form, runs, and gives its bits."""
    sp, g = problem(m, 11, 20, 200, 6, 0.3, 1.5)
    plain = run_anch(m, host_pileup(m, sp), g, A2, 2)
    monkeypatch.setenv("DMX_FORCE_CHECK", "1")
    forced = run_anch(m, host_pileup(m, sp), g, A2, 2)
    for k in ("anchors", "c0", "pairs", "llks00"):
        assert np.array_equal(forced[k], plain[k]), k
    assert forced["summary"].tobytes() == plain["summary"].tobytes()


def test_results_that_cannot_fit_are_refused_before_anything_is_allocated(m):
    """V = 4 094, the engine's widest pool, T = 8, and an empty pileup of so many barcodes that c0 and pairs exceed the free memory:
    DMX_ERR_NOMEM, the earlier result of the same engine is still there, and a small call afterwards is right."""
    capi, E = m["capi"], m["engine"]
    rng = np.random.default_rng(41)
    S, V, B = 6, 4094, 3
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = QM.genotypes(E, rng, raw.alleles, "GT")
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.8, 2.0, doublet_rate=0.3)
    free = m["torch"].cuda.mem_get_info(0)[0]
    per_barcode = 8 * (V * 2 + 8 * V * 2)                      # c0[V][2] and pairs[8][V][2][1] in bytes
    nb = int(free // per_barcode) + 1024
    po = np.zeros(nb + 1, dtype=np.int64)
    zi = np.zeros(nb, dtype=np.int32)
    e = E.Engine(V, A2, 0.5)
    try:
        e.set_genotypes(g)
        e.set_pileup(host_pileup(m, sp))
        e.doublet_anchored(8)
        first = e.get_anchored()
        assert first["pairs"].shape == (B, 8, V, 2, 1) and first["pairs"].any()
        e.set_pileup(E.HostPileup(nb, S, po, po, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), zi, zi, zi))
        with pytest.raises(capi.DmxError) as ei:
            e.doublet_anchored(8)
        assert ei.value.code == capi.DMX_ERR_NOMEM
        kept = e.get_anchored()                                  # the refused call touched nothing
        for k in ("anchors", "c0", "pairs", "llks00"):
            assert np.array_equal(kept[k], first[k]), k
        assert kept["summary"].tobytes() == first["summary"].tobytes()
        e.set_pileup(host_pileup(m, sp))
        e.doublet_anchored(2)
        small = e.get_anchored()
        assert np.array_equal(small["c0"], first["c0"]) and np.array_equal(small["pairs"], first["pairs"][:, :2])
        assert np.array_equal(small["anchors"], first["anchors"][:, :2])
    finally:
        e.close()


def e2e_pool(m, seed, B, S, V, delta, soft=False):
    return AR.e2e_pool(m["synth"], m["engine"], seed, B, S, V, delta, soft)


E2E_POOLS = AR.E2E_POOLS


def oracle_files(oracle, sp, g, alphas, barcodes, samples, prefix):
    return oracle.run_csr(QM.oracle_csr(oracle, sp, barcodes), list(samples), g, oracle.Params(tuple(alphas), 0.5, 0, 0, 0, False), str(prefix))


@pytest.mark.parametrize("seed,B,S,V,delta,alphas,soft", E2E_POOLS)
def test_files_end_to_end(m, oracle, tmp_path, seed, B, S, V, delta, alphas, soft):
    sp, g = e2e_pool(m, seed, B, S, V, delta, soft)
    barcodes = [m["synth"].barcode_name(c) for c in range(B)]
    samples = [f"S-{j}" for j in range(V)]
    ref = oracle_files(oracle, sp, g, alphas, barcodes, samples, tmp_path / "ref")
    n_pairs = np.diff(sp.cell_pair_off)
    dt = m["capi"].SUMMARY_DTYPE
    recs = {}
    for b in range(B):                                 # the precondition, with no barcode left out
        if n_pairs[b] == 0:
            continue
        anc, recs[b] = AR.record(ref.llksAB[b], ref.llks00[b], alphas, 0.5, int(n_pairs[b]), dt, T=2)
        assert AR.donor_among(ref.llksAB[b], anc) and not AR.missed(ref.llksAB[b], alphas, anc), b
    pl = host_pileup(m, sp)
    m["anchored"].anchored_run(pl, g, samples, alphas, str(tmp_path / "anc"), n_anchor=2, barcodes=barcodes)
    m["engine"].demuxlet_run(pl, g, samples, alphas, str(tmp_path / "full"), barcodes=barcodes)
    assert (tmp_path / "anc.sing2").read_bytes() == (tmp_path / "ref.sing2").read_bytes()
    assert (tmp_path / "anc.single").read_bytes() == (tmp_path / "full.single").read_bytes()
    got = [l.split("\t") for l in (tmp_path / "anc.best").read_text().splitlines()]
    want = [l.split("\t") for l in (tmp_path / "ref.best").read_text().splitlines()]
    assert got[0] == want[0] and len(got) == len(want)
    ip, ib = got[0].index("PRB.DBL"), got[0].index("BARCODE")
    cell = {bc: c for c, bc in enumerate(barcodes)}
    for x, y in zip(got[1:], want[1:]):
        assert x[:ip] + x[ip + 1:] == y[:ip] + y[ip + 1:], (x, y)
        assert x[ip] == "%.3g" % AR.ratios(recs[cell[x[ib]]])[0], (x, y)
    head = (tmp_path / "anc.anchors.tsv").read_text().splitlines()
    assert head[0].split("\t") == ["BARCODE", "N.SNP", "ANCHOR.1", "ANCHOR.2", "N.ENTRY"] and len(head) == 1 + int((n_pairs > 0).sum())


@pytest.mark.parametrize("T,alphas", [(2, A2), (4, A2), (2, (0.0, 0.25, 0.5))])
def test_low_depth_pool_through_verify(m, oracle, tmp_path, T, alphas):
    """About 30 SNPs per barcode: --verify names as SAME.PAIR = 0 exactly the barcodes whose best entry the restatement on the oracle's
    grid says lies outside D_b (the order of the donors ignored at alpha 0.5 only: the A = 3 case has best entries at alpha 0.25), and
    PRB.DBL.ANCHORED never exceeds PRB.DBL.FULL."""
    B, S, V = 200, 3000, 16
    sp, g = e2e_pool(m, 205, B, S, V, 0.01)
    barcodes = [m["synth"].barcode_name(c) for c in range(B)]
    samples = [f"S-{j}" for j in range(V)]
    ref = QM.oracle_run(oracle, sp, g, alphas)
    n_pairs = np.diff(sp.cell_pair_off)
    want_missed = set()
    for b in np.flatnonzero(n_pairs > 0):
        anc = AR.choose_anchors(ref.llksAB[b][:, 0, 0], T)
        if AR.missed(ref.llksAB[b], alphas, anc):
            want_missed.add(barcodes[b])
    r = m["anchored"].anchored_run(host_pileup(m, sp), g, samples, alphas, str(tmp_path / "a"), n_anchor=T, verify=B, seed=1, barcodes=barcodes)
    rows = [l.split("\t") for l in (tmp_path / "a.anchored_check.tsv").read_text().splitlines()]
    assert "\t".join(rows[0]) + "\n" == m["anchored"].CHECK_HEADER
    assert len(rows) - 1 == int((n_pairs > 0).sum()) == r["check"]["n_verified"]
    got_missed = {x[0] for x in rows[1:] if x[4] == "0"}
    print(f"T={T} A={len(alphas)}: missed {sorted(got_missed)}, expected {sorted(want_missed)}")
    assert got_missed == want_missed
    assert r["check"]["n_same_pair"] == len(rows) - 1 - len(want_missed)
    s = r["summary"]
    full = {x[0]: float(x[5]) for x in rows[1:]}
    for b in np.flatnonzero(n_pairs > 0):
        assert AR.ratios(s[b])[0] <= full[barcodes[b]] * (1 + 1e-5) + 1e-12            # (the file rounds PRB.DBL.FULL to six digits)
    # the exact statement, on the records: run the full grid here and compare PRB.DBL unrounded
    grid, l00, summ = run_full(m, host_pileup(m, sp), g, alphas)
    for b in np.flatnonzero(n_pairs > 0):
        assert AR.ratios(s[b])[0] <= AR.ratios(summ[b])[0] + 1e-12, b


def test_command_line(m, tmp_path):
    sp, g = e2e_pool(m, 3, 40, 600, 10, 0.1)
    refine, A = m["refine"], m["anchored"]
    samples = [f"S-{j}" for j in range(10)]
    barcodes = [m["synth"].barcode_name(c) for c in range(40)]
    dump = tmp_path / "x.pileup.txt"
    refine.write_pileup_txt(str(dump), refine.PileupDump(samples, [(1, 100 + 10 * j, "A", "C") for j in range(600)], g, barcodes, host_pileup(m, sp)))
    assert A.main(["--pileup", str(dump), "--out", str(tmp_path / "d"), "--anchors", "3", "--verify", "10", "--seed", "4"]) == 0
    for ext in (".best", ".single", ".sing2", ".anchors.tsv", ".anchored_check.tsv"):
        assert (tmp_path / ("d" + ext)).exists()
    assert len((tmp_path / "d.anchored_check.tsv").read_text().splitlines()) == 11
    assert len((tmp_path / "d.anchors.tsv").read_text().splitlines()[0].split("\t")) == 6
    assert A.main(["--pileup", str(dump), "--out", str(tmp_path / "n"), "--no-arbiter"]) == 0
    m["engine"].demuxlet_run(host_pileup(m, sp), g, samples, A2, str(tmp_path / "f"), barcodes=barcodes)
    assert (tmp_path / "n.sing2").read_bytes() == (tmp_path / "f.sing2").read_bytes() == (tmp_path / "d.sing2").read_bytes()
