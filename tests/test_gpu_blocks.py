"""GPU (-m gpu): block-resolved likelihoods (Engine.block_llk / dmx_engine_block_llk; blocks.block_run).

The yardstick is the existing STRICT grid of Engine.run() / get_doublet() — which the goldens pin to the reference within 1e-9 — never
the new code: with G = 1 every value is that grid's entry, bit for bit; for any G, block g's values are the STRICT grid of a fresh engine
staged with sites.drop_snps of everything outside block g.  Then: block sums add up within the reordering bound, the bits do not depend
on the call, the refusals, and the three scenarios of tests/blocks_scenarios.py end to end through blocks.block_run.

Shapes: B <= 40 barcodes on S = 300 SNPs.  Barcodes 0..6 hold 0, 1, 31, 32, 33, 64 and 65 pairs (the tile is 32 pairs), barcode 7 lies
inside SNPs [200, 240); depths 0 (a pair whose only read had allele 2 stores no read) to 17 (more than four stored reads)."""
import numpy as np
import pytest

import blocks_scenarios as SC
import unsafe_geno as UG

pytestmark = pytest.mark.gpu
S = 300
COUNTS = (0, 1, 31, 32, 33, 64, 65, 20, 5, 40, 17, 90, 2, 48)
DEPTHS = np.array([0, 1, 1, 1, 1, 2, 2, 3, 5, 6, 17])
A_OF = {2: (0.0, 0.5), 3: (0.0, 0.3, 0.5)}
CONFIGS = [(2, 2, 0), (5, 3, 1), (8, 2, 8), (33, 3, 8), (33, 2, 1)]       # V, A, E


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import blocks, build, capi, engine, sites, synth
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return dict(torch=torch, capi=capi, engine=engine, sites=sites, synth=synth, blocks=blocks)


def craft_cells(rng, alleles, counts):
    """Per barcode (snps, nrd, reads): barcode c is sample c mod V mixed with sample (c + 1) mod V for every third barcode."""
    Sn, V, _ = alleles.shape
    dosage = np.clip(alleles, 0, 1).sum(axis=2)
    cells = []
    for c, n in enumerate(counts):
        lo, hi = (200, 240) if c == 7 else (0, Sn)
        snps = np.sort(rng.choice(np.arange(lo, hi), size=n, replace=False)).astype(np.int32)
        nrd = rng.choice(DEPTHS, size=n)
        pr = np.repeat(np.arange(n), nrd)
        src = np.where((c % 3 == 2) & (rng.random(len(pr)) < 0.5), (c + 1) % V, c % V)
        alt = rng.random(len(pr)) < dosage[snps[pr], src] / 2.0
        bq = rng.integers(13, 41, size=len(pr)).astype(np.uint8)
        cells.append((snps, nrd.astype(np.uint8), (bq | (alt.astype(np.uint8) << 7)).astype(np.uint8)))
    return cells


def assemble(m, cells, order=None):
    order = range(len(cells)) if order is None else order
    sel = [cells[c] for c in order]
    B = len(sel)
    cpo = np.concatenate([[0], np.cumsum([len(x[0]) for x in sel])]).astype(np.int64)
    cro = np.concatenate([[0], np.cumsum([len(x[2]) for x in sel])]).astype(np.int64)
    cat = lambda i, dt: np.ascontiguousarray(np.concatenate([x[i] for x in sel]).astype(dt)) if B else np.zeros(0, dtype=dt)
    tot = np.diff(cro).astype(np.int32)
    return m["engine"].HostPileup(B, S, cpo, cro, cat(0, np.int32), cat(1, np.uint8), cat(2, np.uint8), tot, tot.copy(), tot.copy())


_PROBLEMS = {}


def problem(m, V, A, B=len(COUNTS)):
    """Cells, genotypes, pileup and the STRICT grid of one (V, A), computed once."""
    key = (V, A, B)
    if key not in _PROBLEMS:
        rng = np.random.default_rng(4100 + 10 * V + A)
        raw = m["synth"].make_raw_genotypes(rng, S, V)
        g = np.stack([m["engine"].geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
        counts = list(COUNTS) + list(rng.integers(0, 70, size=B - len(COUNTS)))
        cells = craft_cells(rng, raw.alleles, counts)
        pl = assemble(m, cells)
        grid, l00 = strict_grid(m, pl, g, A_OF[A])
        for a in (grid, l00):
            a.setflags(write=False)
        _PROBLEMS[key] = dict(cells=cells, g=g, pl=pl, grid=grid, l00=l00, alphas=A_OF[A], V=V, A=A)
    return _PROBLEMS[key]


def strict_grid(m, pl, g, alphas):
    e = m["engine"].Engine(g.shape[1], alphas, 0.5, mode=m["capi"].DMX_MODE_STRICT)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        e.run()
        grid, l00, _ = e.get_doublet()
    finally:
        e.close()
    return grid, l00


def make_extra(rng, B, E, V, A):
    """Random entries: about a sixth unused, about a sixth on the diagonal."""
    ex = np.stack([rng.integers(0, V, size=(B, E)), rng.integers(0, V, size=(B, E)), rng.integers(0, A, size=(B, E))], axis=2).astype(np.int32)
    u = rng.random((B, E))
    ex[u < 1 / 6] = (-1, 0, 0)
    d = (u >= 1 / 6) & (u < 1 / 3)
    ex[d, 1] = ex[d, 0]
    return ex


def run_blocks(m, pl, g, alphas, block, G, extra=None, mode=None, n_extra=None):
    e = m["engine"].Engine(g.shape[1], alphas, 0.5, mode=m["capi"].DMX_MODE_STRICT if mode is None else mode)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        return e.block_llk(block, G, extra, n_extra)
    finally:
        e.close()


def grid_entries(grid, extra):
    """ext[b][s] the grid would give: grid[b][j][k][n], 0 for an unused slot."""
    B, E, _ = extra.shape
    out = np.zeros((B, E))
    for b in range(B):
        for s in range(E):
            j, k, n = extra[b, s]
            if j >= 0:
                out[b, s] = grid[b, j, k, n]
    return out


def block_ids(cuts, ids, n=S):
    """block[n]: SNP i belongs to run r = the number of cuts <= i, whose id is ids[r]."""
    return np.asarray(ids, dtype=np.int32)[np.searchsorted(np.asarray(cuts), np.arange(n), side="right")]


def cuts_of(p):
    """Cuts from barcode 6 (65 pairs): at the SNP of its pair 32 (a tile boundary), of its pair 10 (mid-tile) and of its pair 41, which is
    also between two consecutive pairs of that barcode; none inside [200, 240), where barcode 7 lives."""
    sn = p["cells"][6][0]
    c = sorted({int(sn[10]), int(sn[32]), int(sn[41]), int(sn[50]), 297, 299})
    c = [x for x in c if not 200 < x < 240]
    assert len(set(c)) >= 4
    return c


@pytest.mark.parametrize("V,A,E", CONFIGS)
@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_one_block_is_the_grid(m, V, A, E, mode):
    p = problem(m, V, A)
    B = p["pl"].n_cells
    ex = make_extra(np.random.default_rng(5), B, E, V, A)
    r = run_blocks(m, p["pl"], p["g"], p["alphas"], np.zeros(S, dtype=np.int32), 1, ex if E else None,
                   mode=m["capi"].DMX_MODE_FAST if mode == "fast" else None)
    assert r["col"].shape == (B, 1, V) and r["l00"].shape == (B, 1, A) and r["ext"].shape == (B, 1, E)
    assert np.array_equal(r["col"][:, 0], p["grid"][:, :, 0, 0])
    assert np.array_equal(r["l00"][:, 0], p["l00"])
    assert np.array_equal(r["ext"][:, 0], grid_entries(p["grid"], ex))
    assert np.array_equal(r["n_snp"][:, 0], np.diff(p["pl"].cell_pair_off))


def check_block_is_sub_pileup(m, p, block, r, ex, g_list):
    for gid in g_list:
        sub = m["sites"].drop_snps(p["pl"], block != gid)
        grid, l00 = strict_grid(m, sub, p["g"], p["alphas"])
        assert np.array_equal(r["col"][:, gid], grid[:, :, 0, 0]), gid
        assert np.array_equal(r["l00"][:, gid], l00), gid
        assert np.array_equal(r["ext"][:, gid], grid_entries(grid, ex)), gid
        assert np.array_equal(r["n_snp"][:, gid], np.diff(sub.cell_pair_off)), gid


@pytest.mark.parametrize("V,A,E", CONFIGS)
def test_a_block_is_a_sub_pileup(m, V, A, E):
    p = problem(m, V, A)
    B = p["pl"].n_cells
    ex = make_extra(np.random.default_rng(6), B, E, V, A)
    cuts = cuts_of(p)
    cell_snp = np.repeat(np.arange(B), np.diff(p["pl"].cell_pair_off))
    # G = 2: the one cut is the tile boundary of barcode 6.  G = 7: five runs with the ids 0, 1, 3, 4, 6 (2 and 5 have no SNP)
    for G, cc, ids in ((2, [int(p["cells"][6][0][32])], [0, 1]), (7, cuts[:4], [0, 1, 3, 4, 6])):
        block = block_ids(cc, ids)
        assert np.all(np.diff(block) >= 0)
        assert len(set(block[p["cells"][7][0]])) == 1                                    # barcode 7 lies inside one block
        r = run_blocks(m, p["pl"], p["g"], p["alphas"], block, G, ex if E else None)
        want_n = np.zeros((B, G), dtype=np.int64)
        np.add.at(want_n, (cell_snp, block[p["pl"].pair_snp]), 1)
        assert np.array_equal(r["n_snp"], want_n)
        check_block_is_sub_pileup(m, p, block, r, ex, ids)
        for gid in set(range(G)) - set(ids):
            assert not r["col"][:, gid].any() and not r["l00"][:, gid].any() and not r["ext"][:, gid].any() and not r["n_snp"][:, gid].any()
        unc = r["n_snp"] == 0
        assert unc.any() and not r["col"][unc].any() and not np.signbit(r["col"][unc]).any()


@pytest.mark.parametrize("V,A,E", [(8, 2, 8), (33, 3, 1)])
def test_one_snp_per_block_and_the_sums_add_up(m, V, A, E):
    """G = S: three blocks chosen with a fixed seed are compared with their sub-pileups.  The G = S values are the terms themselves, so the
    sum over g of col must lie within 2 (n - 1) 2^-53 sum |term| of the G = 1 value (the standard reordering bound), and so must G = 7's."""
    p = problem(m, V, A)
    B = p["pl"].n_cells
    ex = make_extra(np.random.default_rng(7), B, E, V, A)
    block = np.arange(S, dtype=np.int32)
    r = run_blocks(m, p["pl"], p["g"], p["alphas"], block, S, ex)
    covered = np.flatnonzero(r["n_snp"].sum(axis=0) >= 3)
    pick = np.random.default_rng(8).choice(covered, size=3, replace=False)
    check_block_is_sub_pileup(m, p, block, r, ex, [int(x) for x in pick])
    assert r["n_snp"].max() == 1
    n = r["n_snp"].sum(axis=1)[:, None]
    bound = 2.0 * np.maximum(n - 1, 0) * 2.0 ** -53 * np.abs(r["col"]).sum(axis=1)
    whole = p["grid"][:, :, 0, 0]
    r7 = run_blocks(m, p["pl"], p["g"], p["alphas"], block_ids(cuts_of(p)[:4], [0, 1, 3, 4, 6]), 7, ex)
    for name, x in (("G = S", r["col"]), ("G = 7", r7["col"])):
        d = np.abs(x.sum(axis=1) - whole)
        print(name, "max |sum - whole| / bound", float(np.max(d / np.where(bound > 0, bound, 1.0))))
        assert np.all(d <= bound), name


def test_bits_do_not_depend_on_the_call(m):
    V, A, E = 8, 2, 8
    p = problem(m, V, A, B=40)
    pl, g, alphas, cells = p["pl"], p["g"], p["alphas"], p["cells"]
    B = pl.n_cells
    ex = make_extra(np.random.default_rng(9), B, E, V, A)
    block = block_ids(cuts_of(p)[:4], [0, 1, 3, 4, 6])
    torch = m["torch"]
    e = m["engine"].Engine(V, alphas, 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        e.run()
        before = (e.get_singlet(), e.get_doublet())
        r = e.block_llk(block, 7, ex)
        again = e.block_llk(block, 7, ex)                                                # a repeat call
        d_ex = torch.from_numpy(ex).cuda()
        dev = e.block_llk(block, 7, int(d_ex.data_ptr()), n_extra=E)                     # extra from device memory
        none = e.block_llk(block, 7)                                                     # E = 0
        asg = (np.arange(B) % V).astype(np.int32)
        e.ambient_profile(asg, np.full(S, 0.3), np.array([0.0, 0.1]))
        after_amb = e.block_llk(block, 7, ex)                                            # after an ambient profile
        after = (e.get_singlet(), e.get_doublet())
    finally:
        e.close()
    for other in (again, dev, after_amb):
        for k in ("col", "l00", "ext", "n_snp"):
            assert np.array_equal(other[k], r[k]), k
    assert none["ext"].shape == (B, 7, 0)
    for k in ("col", "l00", "n_snp"):
        assert np.array_equal(none[k], r[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0]))
    assert np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1]) and before[1][2].tobytes() == after[1][2].tobytes()
    assert np.array_equal(before[1][0], p["grid"])
    # a barcode alone, and a permutation of the barcodes
    for c in (6, 11):
        one = run_blocks(m, assemble(m, cells, [c]), g, alphas, block, 7, ex[[c]])
        for k in ("col", "l00", "ext", "n_snp"):
            assert np.array_equal(one[k][0], r[k][c]), (k, c)
    perm = np.random.default_rng(10).permutation(B)
    pr = run_blocks(m, assemble(m, cells, perm), g, alphas, block, 7, ex[perm])
    for k in ("col", "l00", "ext", "n_snp"):
        assert np.array_equal(pr[k], r[k][perm]), k


def test_refusals(m):
    import ctypes
    capi, E = m["capi"], m["engine"]
    p = problem(m, 5, 3)
    pl, g, alphas = p["pl"], p["g"], p["alphas"]
    B = pl.n_cells
    zero = np.zeros(S, dtype=np.int32)

    def code(fn):
        with pytest.raises(capi.DmxError) as ex:
            fn()
        return ex.value.code, str(ex.value)

    e = E.Engine(5, alphas, 0.5)
    try:
        assert code(lambda: e.block_llk_info())[0] == capi.DMX_ERR_STATE
        assert code(lambda: e.block_llk(zero, 1))[0] == capi.DMX_ERR_STATE               # neither pileup nor genotypes
        e.set_genotypes(g)
        assert code(lambda: e.block_llk(zero, 1))[0] == capi.DMX_ERR_STATE               # genotypes, still no pileup
        e.set_pileup(pl)
        assert e._L.dmx_engine_get_block_llk(e._h, None, None, None, None) == capi.DMX_ERR_STATE      # a query before a call
        good = e.block_llk(zero, 1)
        dec = zero.copy(); dec[100:] = 1; dec[200] = 0
        c, msg = code(lambda: e.block_llk(dec, 2))
        assert c == capi.DMX_ERR_ARG and "decreases" in msg
        for bad in (-1, 2):
            x = zero.copy(); x[-1 if bad > 0 else 0] = bad
            c, msg = code(lambda: e.block_llk(x, 2))
            assert c == capi.DMX_ERR_ARG and "not in [0, 2)" in msg
        assert code(lambda: e.block_llk(zero, 0))[0] == capi.DMX_ERR_ARG                 # G < 1
        assert code(lambda: e.block_llk(zero, 1, np.zeros((B, 9, 3), dtype=np.int32)))[0] == capi.DMX_ERR_ARG       # E = 9
        ok = np.zeros((B, 2, 3), dtype=np.int32)
        for j, k, n in ((5, 0, 0), (0, 5, 0), (0, 0, 3), (-2, 0, 0), (0, -1, 0), (0, 0, -1)):
            x = ok.copy(); x[3, 1] = (j, k, n)
            c, msg = code(lambda: e.block_llk(zero, 1, x))
            assert c == capi.DMX_ERR_ARG and "extra[3][1]" in msg
        assert code(lambda: e.block_llk(zero[:-1], 1))[0] == capi.DMX_ERR_ARG            # n_snps
        rq = capi.BlockLlkRequest(B - 1, S, 1, 0, zero.ctypes.data, None, capi.DMX_MEM_HOST)
        assert e._L.dmx_engine_block_llk(e._h, ctypes.byref(rq)) == capi.DMX_ERR_ARG      # n_cells
        rq = capi.BlockLlkRequest(B, S, 1, 2, zero.ctypes.data, ok.ctypes.data, 7)
        assert e._L.dmx_engine_block_llk(e._h, ctypes.byref(rq)) == capi.DMX_ERR_ARG      # extra_memory
        rq = capi.BlockLlkRequest(B, S, 1, 0, zero.ctypes.data, None, capi.DMX_MEM_HOST, (ctypes.c_int32 * 4)(0, 0, 1, 0))
        assert e._L.dmx_engine_block_llk(e._h, ctypes.byref(rq)) == capi.DMX_ERR_ARG      # reserved
        # results that cannot fit: refused before anything is allocated, and the last good result is still there
        c, msg = code(lambda: e.block_llk(zero, 1 << 30))
        assert c == capi.DMX_ERR_NOMEM and "are free" in msg
        col = np.zeros((B, 1, 5))
        assert e._L.dmx_engine_get_block_llk(e._h, col.ctypes.data, None, None, None) == 0
        assert np.array_equal(col, good["col"])
    finally:
        e.close()
    poisoned, _ = UG.poison(g, "zero", np.random.default_rng(0), pl)
    assert not UG.is_safe(poisoned)
    e = E.Engine(5, alphas, 0.5)
    try:
        e.set_genotypes(poisoned); e.set_pileup(pl)
        c, msg = code(lambda: e.block_llk(zero, 1))
        assert c == capi.DMX_ERR_ARG and "no fix-up" in msg and "anchored" in msg
    finally:
        e.close()


@pytest.mark.parametrize("name", ["clean", "soup", "swap"])
def test_scenarios_end_to_end(m, tmp_path, name):
    """The scenarios of blocks_scenarios.py through blocks.block_run: the plain pass, the kernel, the statistics and the three tables."""
    blocks = m["blocks"]
    sc = SC.scenario(m["engine"], m["synth"], name)
    r = blocks.block_run(sc["pl"], sc["g"], sc["sample_ids"], str(tmp_path / "o"), snps=SC.snp_table(), n_blocks=SC.G, barcodes=sc["barcodes"],
                         alphas=SC.ALPHAS)
    assert np.array_equal(r["block"], sc["block"]) and r["info"]["n_blocks"] == SC.G and r["info"]["kernel_ms"] > 0
    rows, st = r["rows"], r["calls"]
    assert rows.has_row.all()
    labels = [blocks.loo_label(rows, b, st["loo_call"][b], SC.ALPHAS, sc["sample_ids"]) for b in range(sc["pl"].n_cells)]
    print(name, SC.check_outcome(name, sc, rows.kind, rows.sng1, st, labels, r["donors"]), r["flags"])
    calls = (tmp_path / "o.block_calls.tsv").read_text().splitlines()
    assert calls[0] + "\n" == blocks.CALLS_HEADER and len(calls) == 1 + sc["pl"].n_cells
    assert (tmp_path / "o.blocks.tsv").read_text().splitlines()[1] == "0\t1\t1\t99001\t100"
    assert (tmp_path / "o.block_donors.tsv").read_text().startswith(blocks.DONORS_HEADER)
    best = (tmp_path / "o.best").read_text()
    blocks.block_run(sc["pl"], sc["g"], sc["sample_ids"], str(tmp_path / "p"), snps=SC.snp_table(), n_blocks=SC.G, barcodes=sc["barcodes"],
                     alphas=SC.ALPHAS, best=str(tmp_path / "o.best"))
    assert (tmp_path / "o.best").read_text() == best and not (tmp_path / "p.best").exists()
    assert (tmp_path / "p.block_calls.tsv").read_text() == (tmp_path / "o.block_calls.tsv").read_text()
