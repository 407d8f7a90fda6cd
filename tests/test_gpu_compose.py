"""GPU (-m gpu): the pileup composer (Engine.compose / dmx_engine_compose) and demuxlet_amd.simulate.

The composer is all-integer, so every check against the restatement of tests/compose_ref.py is an equality: the five arrays and the info
counts over dense and sparse sources of every nrd_width, nearly empty pools, parents of several 64-pair tiles, the width change at
200 + 200 reads, n_out = 1 and n_out = 3 B.  Then the bits (repeat, chunks by index_base, dense against sparse, a parent reproduced and
run), adoption by a second engine against the host copy, no interference with the source engine's results, the argument and state
errors, and simulate_run end to end against the synthetic truth."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import compose_ref as R

pytestmark = pytest.mark.gpu
ALL = 1 << 32
ROOT = Path(__file__).resolve().parents[1]
KEEPS = np.array([0, ALL, 1 << 31, 1 << 30, 3 << 30, round(0.1 * ALL), round(0.03 * ALL)], dtype=np.uint64)


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import build, capi, engine, refine, simulate, synth
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return dict(capi=capi, engine=engine, refine=refine, sim=simulate, synth=synth)


def host_pileup(m, sp, width=None, sparse=False):
    nrd = np.asarray(sp.pair_nrd)
    if width is not None:
        nrd = nrd.astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[width])
    snp = sp.pair_snp
    if sparse and snp is None:
        snp = np.tile(np.arange(sp.n_snps, dtype=np.int32), sp.n_cells)
    return m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, snp, nrd, sp.reads, sp.rd_totl, sp.rd_pass, sp.rd_uniq)


def gt_matrix(m, raw):
    return np.stack([m["engine"].geno_from_gt(raw.alleles[s], 0.01) for s in range(raw.alleles.shape[0])])


def problem(m, seed, B, S, delta, rbar, V=4, dense=False, doublet_rate=0.1):
    rng = np.random.default_rng(seed)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, delta, rbar, dense_layout=dense, doublet_rate=doublet_rate)
    return sp, gt_matrix(m, raw)


def recipe(seed, B, n_out):
    rng = np.random.default_rng(seed)
    par = np.stack([rng.integers(0, B, size=n_out), rng.integers(0, B, size=n_out)], axis=1).astype(np.int32)
    par[rng.random(n_out) < 0.2, 1] = -1
    same = rng.random(n_out) < 0.1
    par[same, 1] = par[same, 0]
    keep = KEEPS[rng.integers(0, len(KEEPS), size=(n_out, 2))]
    return par, keep


def staged(m, g, pl):
    e = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    e.set_genotypes(g)
    e.set_pileup(pl)
    return e


def compose(m, g, pl, par, keep, seed, base=0):
    e = staged(m, g, pl)
    try:
        info = e.compose(par, keep, seed, index_base=base)
        return e.get_composed(), info
    finally:
        e.close()


def same_pileup(a, b):
    return (a.n_cells == b.n_cells and np.array_equal(a.cell_pair_off, b.cell_pair_off) and np.array_equal(a.cell_read_off, b.cell_read_off)
            and np.array_equal(a.pair_snp, b.pair_snp) and a.pair_nrd.dtype == b.pair_nrd.dtype and np.array_equal(a.pair_nrd, b.pair_nrd)
            and np.array_equal(a.reads, b.reads))


def check(m, g, pl, par, keep, seed, base=0):
    hp, info = compose(m, g, pl, par, keep, seed, base)
    ref = R.compose(pl, par, keep, seed, base)
    assert np.array_equal(hp.cell_pair_off, ref["cell_pair_off"]) and np.array_equal(hp.cell_read_off, ref["cell_read_off"])
    assert np.array_equal(hp.pair_snp, ref["pair_snp"])
    assert hp.pair_nrd.dtype == ref["pair_nrd"].dtype and np.array_equal(hp.pair_nrd, ref["pair_nrd"])
    assert np.array_equal(hp.reads, ref["reads"])
    assert info["n_out"] == len(par) == hp.n_cells and info["n_pairs"] == len(ref["pair_snp"]) and info["n_reads"] == len(ref["reads"])
    assert info["nrd_width"] == ref["nrd_width"] and info["bytes_read"] > 0 and info["bytes_written"] >= info["n_pairs"] * 5 + info["n_reads"]
    assert info["count_ms"] > 0 and info["scan_ms"] > 0 and info["fill_ms"] > 0
    assert np.array_equal(hp.rd_totl, np.diff(ref["cell_read_off"])) and np.array_equal(hp.rd_uniq, hp.rd_totl) and np.array_equal(hp.rd_pass, hp.rd_totl)
    return hp, info


# ---- equality with the restatement -------------------------------------------------------------------------------------------------------

def test_dense_source_width_1(m):
    sp, g = problem(m, 1, 60, 257, 1.0, 1.5, dense=True)
    assert sp.pair_snp is None and sp.pair_nrd.dtype == np.uint8 and (np.asarray(sp.pair_nrd) == 0).any()      # zero-read pairs occur
    par, keep = recipe(11, 60, 90)
    hp, info = check(m, g, host_pileup(m, sp), par, keep, seed=101)
    assert info["nrd_width"] == 1 and info["n_pairs"] > 0


def test_sparse_source_width_2(m):
    sp, g = problem(m, 2, 100, 900, 0.3, 1.6)
    par, keep = recipe(12, 100, 100)
    hp, info = check(m, g, host_pileup(m, sp, width=2), par, keep, seed=102)
    assert info["nrd_width"] == 2 and hp.pair_nrd.dtype == np.uint16


def test_sparse_source_width_4(m):
    sp, g = problem(m, 3, 40, 300, 0.4, 2.0)
    par, keep = recipe(13, 40, 60)
    hp, info = check(m, g, host_pileup(m, sp, width=4), par, keep, seed=(1 << 63) + 5)
    assert info["nrd_width"] == 4 and hp.pair_nrd.dtype == np.uint32


def test_pool_where_most_barcodes_have_no_pair(m):
    sp, g = problem(m, 4, 150, 200, 0.002, 1.2)
    assert (np.diff(sp.cell_pair_off) == 0).mean() > 0.5
    par, keep = recipe(14, 150, 200)
    check(m, g, host_pileup(m, sp), par, keep, seed=104)


def test_parents_of_several_tiles(m):
    sp, g = problem(m, 5, 24, 400, 0.5, 1.4)
    assert np.diff(sp.cell_pair_off).min() >= 130
    par, keep = recipe(15, 24, 48)
    par[:6, 1] = (par[:6, 0] + 1) % 24                 # two long parents each, kept whole and thinned: boundaries inside the merge
    keep[:3] = ALL
    hp, info = check(m, g, host_pileup(m, sp), par, keep, seed=105)
    assert np.diff(hp.cell_pair_off).max() > 256


def deep_pileup(m):
    """four barcodes of 30 SNPs each; SNP 6 (and SNP 20 of two of them) holds 200 reads"""
    rng = np.random.default_rng(6)
    po, ro, snp, nrd, reads = [0], [0], [], [], []
    for c in range(4):
        for s in sorted(set(rng.choice(30, size=12, replace=False).tolist()) | {6} | ({20} if c < 2 else set())):
            n = 200 if s == 6 or (s == 20 and c < 2) else int(rng.integers(0, 4))
            snp.append(s); nrd.append(n); reads.extend(rng.integers(0, 256, size=n).tolist())
        po.append(len(snp)); ro.append(len(reads))
    z = np.zeros(4, dtype=np.int32)
    return m["engine"].HostPileup(4, 30, np.array(po, dtype=np.int64), np.array(ro, dtype=np.int64), np.array(snp, dtype=np.int32),
                                  np.array(nrd, dtype=np.uint8), np.array(reads, dtype=np.uint8), z, z.copy(), z.copy())


def test_width_changes_at_200_plus_200_reads(m):
    pl = deep_pileup(m)
    g = gt_matrix(m, m["synth"].make_raw_genotypes(np.random.default_rng(6), 30, 4))
    par = np.array([[0, 1], [2, 3], [1, 1], [3, -1], [0, 2]], dtype=np.int32)
    keep = np.array([[ALL, ALL], [ALL, 3 << 30], [ALL, ALL], [ALL, 0], [1 << 31, 1 << 31]], dtype=np.uint64)
    hp, info = check(m, g, pl, par, keep, seed=106)
    assert info["nrd_width"] == 2 and int(hp.pair_nrd.max()) == 400
    hp1, info1 = check(m, g, pl, par[3:], keep[3:], seed=106)          # nothing merged: the source's width stays
    assert info1["nrd_width"] == 1


def test_one_output_and_three_times_the_source(m):
    sp, g = problem(m, 7, 60, 257, 1.0, 1.5, dense=True)
    pl = host_pileup(m, sp)
    par, keep = recipe(17, 60, 180)
    check(m, g, pl, par[:1], keep[:1], seed=107)
    hp, info = check(m, g, pl, par, keep, seed=107)
    assert info["n_out"] == 180 > pl.n_cells


# ---- bits --------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pool(m):
    sp, g = problem(m, 8, 80, 500, 0.35, 1.5)
    par, keep = recipe(18, 80, 96)
    return sp, g, host_pileup(m, sp), par, keep


def test_repeat_and_chunks_give_the_same_barcodes(m, pool):
    sp, g, pl, par, keep = pool
    e = staged(m, g, pl)
    try:
        e.compose(par, keep, 7)
        a = e.get_composed()
        e.compose(par[:5], keep[:5], 8)                                  # something else in between
        e.compose(par, keep, 7)
        b = e.get_composed()
        assert same_pileup(a, b)
        for k0, k1 in ((0, 31), (31, 32), (32, 96)):
            e.compose(par[k0:k1], keep[k0:k1], 7, index_base=k0)
            c = e.get_composed()
            p0, p1, r0, r1 = (int(x) for x in (a.cell_pair_off[k0], a.cell_pair_off[k1], a.cell_read_off[k0], a.cell_read_off[k1]))
            assert np.array_equal(c.cell_pair_off, a.cell_pair_off[k0:k1 + 1] - p0) and np.array_equal(c.cell_read_off, a.cell_read_off[k0:k1 + 1] - r0)
            assert np.array_equal(c.pair_snp, a.pair_snp[p0:p1]) and np.array_equal(c.pair_nrd, a.pair_nrd[p0:p1]) and np.array_equal(c.reads, a.reads[r0:r1])
    finally:
        e.close()


def test_dense_and_sparse_sources_give_the_same_output(m):
    sp, g = problem(m, 9, 30, 257, 1.0, 1.5, dense=True)
    par, keep = recipe(19, 30, 40)
    a, _ = compose(m, g, host_pileup(m, sp), par, keep, 9)
    b, _ = compose(m, g, host_pileup(m, sp, sparse=True), par, keep, 9)
    c, _ = compose(m, g, host_pileup(m, sp, width=2, sparse=True), par, keep, 9)
    assert same_pileup(a, b)
    assert np.array_equal(a.pair_nrd, c.pair_nrd) and np.array_equal(a.reads, c.reads) and np.array_equal(a.pair_snp, c.pair_snp)


def run_results(e):
    e.run()
    llks, llk0s = e.get_singlet()
    _, l00, summ = e.get_doublet(want_grid=False)
    return llks, llk0s, l00, summ


def same_results(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_one_parent_kept_whole_reproduces_it_and_runs_to_the_same_bits(m, pool):
    sp, g, pl, _, _ = pool
    cells = np.array([5, 5, 79, 0, 33, 12, 47], dtype=np.int32)
    par = np.stack([cells, np.full(len(cells), -1)], axis=1).astype(np.int32)
    keep = np.tile(np.array([ALL, ALL], dtype=np.uint64), (len(cells), 1))
    src = staged(m, g, pl)
    dst = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    try:
        before = run_results(src)
        src.compose(par, keep, 3)
        hp = src.get_composed()
        for k, c in enumerate(cells):
            p0, p1, r0, r1 = (int(x) for x in (pl.cell_pair_off[c], pl.cell_pair_off[c + 1], pl.cell_read_off[c], pl.cell_read_off[c + 1]))
            q0, q1, s0, s1 = (int(x) for x in (hp.cell_pair_off[k], hp.cell_pair_off[k + 1], hp.cell_read_off[k], hp.cell_read_off[k + 1]))
            assert np.array_equal(hp.pair_snp[q0:q1], pl.pair_snp[p0:p1]) and np.array_equal(hp.pair_nrd[q0:q1], pl.pair_nrd[p0:p1])
            assert np.array_equal(hp.reads[s0:s1], pl.reads[r0:r1])
        after = run_results(src)                                         # no interference: the source engine's results stay
        assert same_results(before, after)
        dst.set_genotypes(g)
        dst.set_pileup_struct(src.composed_pileup(), keep=src)
        got = run_results(dst)
        assert got[0].tobytes() == before[0][cells].tobytes() and got[1].tobytes() == before[1][cells].tobytes()
        assert got[2].tobytes() == before[2][cells].tobytes() and got[3].tobytes() == before[3][cells].tobytes()
    finally:
        dst.close(); src.close()


def test_adoption_on_the_device_equals_the_host_copy(m, pool):
    sp, g, pl, par, keep = pool
    src = staged(m, g, pl)
    dev = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    hst = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    try:
        before = run_results(src)
        src.compose(par, keep, 21)
        st = src.composed_pileup()
        assert st.memory == m["capi"].DMX_MEM_DEVICE and st.n_cells == len(par) and not st.rd_totl and st.pair_snp
        dev.set_genotypes(g); dev.set_pileup_struct(st, keep=src)
        hst.set_genotypes(g); hst.set_pileup(src.get_composed())
        assert same_results(run_results(dev), run_results(hst))
        assert same_results(before, run_results(src))
    finally:
        hst.close(); dev.close(); src.close()


def test_errors(m, pool):
    sp, g, pl, par, keep = pool
    capi = m["capi"]
    e = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g)
        for call in (lambda: e.compose(par, keep, 1), e.compose_info, e.composed_pileup, e.get_composed):
            with pytest.raises(capi.DmxError) as ei:
                call()
            assert ei.value.code == capi.DMX_ERR_STATE
        e.set_pileup(pl)
        for call in (e.compose_info, e.composed_pileup, e.get_composed):
            with pytest.raises(capi.DmxError) as ei:
                call()
            assert ei.value.code == capi.DMX_ERR_STATE
        one, k1 = np.array([[0, -1]], dtype=np.int32), np.array([[ALL, 0]], dtype=np.uint64)
        bad = [(np.array([[pl.n_cells, -1]], dtype=np.int32), k1), (np.array([[-1, 0]], dtype=np.int32), k1), (np.array([[0, -2]], dtype=np.int32), k1),
               (np.array([[0, pl.n_cells]], dtype=np.int32), k1), (one, np.array([[ALL + 1, 0]], dtype=np.uint64)), (one, np.array([[0, ALL + 1]], dtype=np.uint64)),
               (np.zeros((0, 2), dtype=np.int32), np.zeros((0, 2), dtype=np.uint64))]
        for p, k in bad:
            with pytest.raises(capi.DmxError) as ei:
                e.compose(p, k, 1)
            assert ei.value.code == capi.DMX_ERR_ARG
        import ctypes as C
        rq = capi.ComposeRequest(1, 0, 0, None, k1.ctypes.data, 1)
        assert e._L.dmx_engine_compose(e._h, C.byref(rq)) == capi.DMX_ERR_ARG
        rq = capi.ComposeRequest(1, 0, 0, one.ctypes.data, None, 1)
        assert e._L.dmx_engine_compose(e._h, C.byref(rq)) == capi.DMX_ERR_ARG
        rq = capi.ComposeRequest((1 << 24) + 1, 0, 0, one.ctypes.data, k1.ctypes.data, 1)     # refused before the arrays are read
        assert e._L.dmx_engine_compose(e._h, C.byref(rq)) == capi.DMX_ERR_ARG
        with pytest.raises(ValueError):
            e.compose(one, np.zeros((2, 2), dtype=np.uint64), 1)
        e.compose(one, k1, 1)                                            # a failed call leaves the engine usable
        assert e.compose_info()["n_out"] == 1
        e.set_pileup(pl)                                                 # staging again drops the composed pileup
        with pytest.raises(capi.DmxError) as ei:
            e.composed_pileup()
        assert ei.value.code == capi.DMX_ERR_STATE
        e.compose(one, k1, 1)
        e.set_pileup_struct(e.composed_pileup(), keep=None)              # an engine staged on its own composed pileup cannot compose over it
        with pytest.raises(capi.DmxError) as ei:
            e.compose(one, k1, 1)
        assert ei.value.code == capi.DMX_ERR_STATE
    finally:
        e.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
# 8 donors with GT rows, 800 barcodes, 10 % true doublets, ~300 covered SNPs per barcode.  The shape was fixed on seeds 1, 2 and 3: at
# full depth the plain pass calls every true singlet (734 / 714 / 720) and every true doublet (66 / 86 / 80) right and 200 of 200 HET
# rows are found; at F = 0.1 a heterotypic doublet keeps ~70 SNPs and 183 / 183 / 182 of 200 are found.  (At 2 000 SNPs x 0.08 the plain
# pass missed one true doublet on seed 3, at 1 200 x 0.06 several on every seed.)
E2E_V, E2E_B, E2E_S, E2E_DELTA, E2E_RBAR, E2E_SEED, E2E_N = 8, 800, 3000, 0.1, 1.2, 1, 200


@pytest.fixture(scope="module")
def e2e(m, tmp_path_factory):
    d = tmp_path_factory.mktemp("sim")
    rng = np.random.default_rng(E2E_SEED)
    raw = m["synth"].make_raw_genotypes(rng, E2E_S, E2E_V)
    sp = m["synth"].make_pileup(rng, raw.alleles, E2E_B, E2E_DELTA, E2E_RBAR, doublet_rate=0.1)
    g = gt_matrix(m, raw)
    pl = host_pileup(m, sp)
    sm = [f"donor{j}" for j in range(E2E_V)]
    bcs = [m["synth"].barcode_name(i) for i in range(E2E_B)]
    out = str(d / "fn")
    r = m["sim"].simulate_run(pl, g, sm, out, bcs, n=E2E_N, seed=5)
    return dict(dir=d, sp=sp, g=g, pl=pl, sm=sm, bcs=bcs, out=out, r=r)


def sigma(p):
    """the binomial sigma of a rate observed on E2E_N rows whose true rate is p"""
    return float(np.sqrt(p * (1.0 - p) / E2E_N))


def table_row(r, kind, depth):
    return next(t for t in r["table"] if t["kind"] == kind and t["depth"] == depth)


def test_e2e_parents_are_true_singlets_of_their_donor(m, e2e):
    assign, truth = e2e["r"]["assign"], e2e["sp"].truth
    used = np.flatnonzero(assign >= 0)
    assert len(used) > 0.8 * (truth[:, 1] < 0).sum()
    assert (truth[used, 1] == -1).all() and (truth[used, 0] == assign[used]).all()


def test_e2e_rates_against_the_synthetic_truth(m, e2e):
    from demuxlet_amd import ambient
    r, truth = e2e["r"], e2e["sp"].truth
    rows = ambient.read_best_rows(e2e["out"] + ".best", e2e["sm"], e2e["bcs"])
    dbl = np.flatnonzero(truth[:, 1] >= 0)
    right = sum(rows.best[c].startswith("DBL-") and {int(rows.dbl1[c]), int(rows.dbl2[c])} == {int(truth[c, 0]), int(truth[c, 1])} for c in dbl)
    plain = right / len(dbl)
    het1, hom1, sng1 = (table_row(r, k, 1.0) for k in ("HET", "HOM", "SNG"))
    het_low = table_row(r, "HET", 0.1)
    print(f"plain pass: {right}/{len(dbl)} true doublets right; HET at depth 1: {het1['n_ok']}/{het1['n']}, at depth 0.1: {het_low['n_ok']}/{het_low['n']}; "
          f"HOM at 1: ok {hom1['n_ok']} dbl {hom1['n_dbl']}; SNG at 1: ok {sng1['n_ok']} dbl {sng1['n_dbl']}")
    assert het1["n"] == hom1["n"] == sng1["n"] == E2E_N
    # sigma from N alone, at the rate compared against: the plain pass's for (b), the SNG control's for (c).  A rate of exactly 1 or 0
    # leaves no slack: at this shape the plain pass and the control are right every time, so HET and HOM rows have to be too
    assert het1["rate"] >= plain - 3.0 * sigma(plain)                                                              # (b)
    assert abs(hom1["rate"] - sng1["rate"]) <= 3.0 * sigma(sng1["rate"])                                           # (c)
    assert hom1["n_dbl"] <= sng1["n_dbl"] + 3.0 * E2E_N * sigma(sng1["n_dbl"] / E2E_N)
    assert het_low["rate"] < het1["rate"]                                                                          # (d)
    # the recipe's donors are the parents' TRUE donors, so OK is a statement about the truth
    rc = r["recipe"]
    assert (truth[rc["parent"][:, 0], 0] == rc["donor"][:, 0]).all()
    two = rc["parent"][:, 1] >= 0
    assert (truth[rc["parent"][two, 1], 0] == rc["donor"][two, 1]).all()


def test_e2e_files(m, e2e):
    out, r = e2e["out"], e2e["r"]
    for ext in (".best", ".single", ".sing2", ".sim.best", ".sim.single", ".sim.sing2", ".sim.tsv", ".sim.recipe.tsv", ".power.tsv"):
        assert Path(out + ext).exists(), ext
    assert not list(e2e["dir"].glob("*.part*"))
    sim = [x.split("\t") for x in Path(out + ".sim.tsv").read_text().splitlines()]
    best = [x.split("\t") for x in Path(out + ".sim.best").read_text().splitlines()]
    assert sim[0] == m["sim"].SIM_HEADER.rstrip("\n").split("\t") and len(sim) - 1 == 4 * 3 * E2E_N
    by_bc = {t[0]: t for t in best[1:]}
    assert len(by_bc) == len(best) - 1
    col = {n: i for i, n in enumerate(best[0])}
    for t in sim[1:]:
        assert t[0] in by_bc and by_bc[t[0]][col["BEST"]] == t[10] and by_bc[t[0]][col["N.SNP"]] == t[8] and by_bc[t[0]][col["RD.UNIQ"]] == t[9]
    pw = [x.split("\t") for x in Path(out + ".power.tsv").read_text().splitlines()]
    rows = [t for t in pw[1:] if not t[0].startswith("#")]
    assert len(rows) == 12 and [t[0] for t in rows] == ["HET"] * 4 + ["HOM"] * 4 + ["SNG"] * 4
    for t in rows:
        assert int(t[3]) == E2E_N == int(t[4]) + int(t[5]) + int(t[6]) and 0 <= int(t[7]) <= E2E_N
    assert pw[5][0] == "#POOL" and pw[6][0] == "#POOL" and 0.0 < float(pw[6][4]) < 1.0
    # depth shows in the composed barcodes: the median N.SNP falls with F
    med = [float(t[9]) for t in rows[:4]]
    assert med[0] > med[1] > med[2] > med[3] > 0


def test_e2e_chunked_run_gives_the_same_files(m, e2e):
    out2 = str(e2e["dir"] / "chunked")
    m["sim"].simulate_run(e2e["pl"], e2e["g"], e2e["sm"], out2, e2e["bcs"], best=e2e["out"] + ".best", n=E2E_N, seed=5, max_bytes=1 << 20)
    for ext in (".sim.best", ".sim.single", ".sim.sing2", ".sim.tsv", ".power.tsv"):
        assert Path(out2 + ext).read_bytes() == Path(e2e["out"] + ext).read_bytes(), ext


def test_e2e_command_line_gives_the_same_power_table(m, e2e):
    d = e2e["dir"]
    snps = [(0, 100 + s, "A", "C") for s in range(E2E_S)]
    m["refine"].write_pileup_txt(str(d / "pool.pileup.txt"), m["refine"].PileupDump(e2e["sm"], snps, e2e["g"], e2e["bcs"], e2e["pl"]))
    cmd = [sys.executable, "-m", "demuxlet_amd.simulate", "--pileup", str(d / "pool.pileup.txt"), "--out", str(d / "cli"), "--n", str(E2E_N), "--seed", "5"]
    subprocess.run(cmd, check=True, cwd=str(ROOT), timeout=300)
    assert Path(str(d / "cli") + ".power.tsv").read_bytes() == Path(e2e["out"] + ".power.tsv").read_bytes()
    assert Path(str(d / "cli") + ".sim.tsv").read_bytes() == Path(e2e["out"] + ".sim.tsv").read_bytes()
