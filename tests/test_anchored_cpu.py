"""CPU: the anchored doublet search's restatement (tests/anchored_ref.py) against the reference's scans over the oracle's full grids, the
precondition of the GPU end-to-end test on the oracle alone, and the host side of demuxlet_amd/anchored.py (argument rules, the
.anchors.tsv and check-file writers, command-line errors).  No GPU compute is called."""
import numpy as np
import pytest

import anchored_ref as AR
import quality_mix as QM
from golden_util import Golden, summary_from_grid


@pytest.fixture(scope="module")
def mods():
    from demuxlet_amd import anchored, build, capi, engine, synth
    build.build()
    capi.load()
    return dict(anchored=anchored, capi=capi, engine=engine, synth=synth)


@pytest.mark.parametrize("name", ["gt_v4_a2_pair", "pl_v32_a3", "gt_v3_alpha_quirk"])
def test_with_every_sample_an_anchor_the_restatement_is_the_references_scan(mods, oracle, name):
    """D_b with all V samples as anchors is every (j != k, n >= 1): indices and llk fields equal summary_from_grid's, the printed ratios
    to 1e-12 (max_llk may differ: the entries [j][k != 0][0] are not in the anchored maximum).  V = 32 needs explicit anchors beyond the
    engine's eight; the eight chosen ones are checked to be the top of the singlet column."""
    gd = Golden(name)
    csr, out = oracle.run_problem(gd.problem(oracle))
    dt = mods["capi"].SUMMARY_DTYPE
    V = len(gd.sample_ids)
    n_done = 0
    for c in range(csr.n_cells):
        n_pairs = int(csr.cell_off[c + 1] - csr.cell_off[c])
        if n_pairs == 0 or not out.processed[c]:
            continue
        grid, l00 = out.llksAB[c], out.llks00[c]
        want = summary_from_grid(grid, l00, gd.alphas, gd.doublet_prior, n_pairs, dt)
        anc, got = AR.record(grid, l00, gd.alphas, gd.doublet_prior, n_pairs, dt, anchors=np.arange(V))
        for f in AR.INDEX_FIELDS + AR.LLK_FIELDS:
            assert got[f] == want[f], (c, f)
        for x, y in zip(AR.ratios(got), AR.ratios(want)):
            assert abs(x - y) <= 1e-12 * abs(y), (c, x, y)
        top = AR.choose_anchors(grid[:, 0, 0], min(8, V))
        assert len(set(top.tolist())) == len(top) and top[0] == want["i_sing1"] and (V < 2 or top[1] == want["i_sing2"])
        assert np.all(np.diff(grid[top, 0, 0]) <= 0)
        if V <= 8:
            anc8, got8 = AR.record(grid, l00, gd.alphas, gd.doublet_prior, n_pairs, dt, T=V)
            assert sorted(anc8.tolist()) == list(range(V))
            for f in AR.INDEX_FIELDS + AR.LLK_FIELDS + ("max_llk",):
                assert got8[f] == got[f], (c, f)
        n_done += 1
    assert n_done > 0


def test_order_counts_except_at_alpha_half(mods):
    """A = 3: at alpha 0.25 the entries (0, k, n) and (k, 0, n) are different hypotheses — SAME.PAIR and the restatement's `missed` tell them
    apart; at alpha 0.5 they are one, and both ignore the order."""
    A, alphas = mods["anchored"], (0.0, 0.25, 0.5)
    dt = mods["capi"].SUMMARY_DTYPE
    full, anch = np.zeros((), dtype=dt), np.zeros((), dtype=dt)
    full["j_best"], full["k_best"] = 0, 3
    anch["j_best"], anch["k_best"] = 3, 0
    for n, same in ((1, False), (2, True)):
        full["n_best"] = anch["n_best"] = n
        assert A.same_pair(full, anch, alphas) == same
        assert A.same_pair(full, full, alphas) and A.same_pair(anch, anch, alphas)
    anch["n_best"] = 1
    assert not A.same_pair(full, anch, alphas)
    # a grid whose best entry is (0, 3, n) with anchors {1, 2}: (3, 0, n) is in D_b (column 0), (0, 3, n) is not
    for n, miss in ((1, True), (2, False)):
        grid = np.full((5, 5, 3), -50.0)
        grid[0, 3, n] = -1.0
        grid[3, 0, n] = -1.0 - 1e-12
        assert AR.best_entry(grid) == (0, 3, n)
        assert AR.missed(grid, alphas, [1, 2]) == miss
        assert not AR.missed(grid, alphas, [1, 3]) and not AR.donor_among(grid, [1, 2]) and AR.donor_among(grid, [3, 2])
        # ... and the record over D_b names the mirror, which SAME.PAIR counts as the same pair at alpha 0.5 only
        _, rec = AR.record(grid, np.zeros(3), alphas, 0.5, 4, dt, anchors=[1, 2])
        assert (rec["j_best"], rec["k_best"], rec["n_best"]) == (3, 0, n)
        _, ref = AR.record(grid, np.zeros(3), alphas, 0.5, 4, dt, anchors=np.arange(5))
        assert A.same_pair(ref, rec, alphas) == (not miss)


@pytest.mark.parametrize("seed,B,S,V,delta,alphas,soft", AR.E2E_POOLS)
def test_end_to_end_pools_satisfy_their_precondition(mods, oracle, seed, B, S, V, delta, alphas, soft):
    """On the oracle's grid every barcode's best pair has a donor among its top 2 singlets — no barcode left out — and so lies in D_b."""
    sp, g = AR.e2e_pool(mods["synth"], oracle, seed, B, S, V, delta, soft)
    ref = QM.oracle_run(oracle, sp, g, alphas)
    n_pairs = np.diff(sp.cell_pair_off)
    assert (n_pairs > 0).all()
    for b in range(B):
        top2 = AR.choose_anchors(ref.llksAB[b][:, 0, 0], 2)
        assert AR.donor_among(ref.llksAB[b], top2) and not AR.missed(ref.llksAB[b], alphas, top2), b


def test_low_depth_pool_misses_some_pairs(mods, oracle):
    """The low-depth pool of the GPU test has barcodes whose best pair two anchors miss, and fewer with four."""
    seed, B, S, V, delta = AR.LOW_DEPTH_POOL
    sp, g = AR.e2e_pool(mods["synth"], oracle, seed, B, S, V, delta)
    ref = QM.oracle_run(oracle, sp, g)
    cov = np.flatnonzero(np.diff(sp.cell_pair_off) > 0)
    n2 = sum(AR.missed(ref.llksAB[b], (0.0, 0.5), AR.choose_anchors(ref.llksAB[b][:, 0, 0], 2)) for b in cov)
    n4 = sum(AR.missed(ref.llksAB[b], (0.0, 0.5), AR.choose_anchors(ref.llksAB[b][:, 0, 0], 4)) for b in cov)
    print(f"missed at T = 2: {n2}, at T = 4: {n4} of {len(cov)}")
    assert 0 < n4 < n2 < len(cov) // 10


def test_capi_symbols(mods):
    for name in ("dmx_engine_doublet_anchored", "dmx_engine_get_anchored", "dmx_engine_anchored_info"):
        assert name in mods["capi"].SYMBOLS
        assert hasattr(mods["capi"].load(), name)


def test_argument_rules(mods):
    A = mods["anchored"]
    assert A.check_n_anchor(8, 8) == 8 and A.check_n_anchor(1, 2) == 1
    for T, V in ((0, 5), (9, 20), (3, 2), (-1, 4)):
        with pytest.raises(ValueError):
            A.check_n_anchor(T, V)
    assert np.array_equal(A.check_alphas([0.0, 0.5]), [0.0, 0.5])
    for al in ([0.5], [], [0.0, 1.5], [-0.1, 0.5]):
        with pytest.raises(ValueError):
            A.check_alphas(al)
    assert A.entries_per_barcode(np.array([[3, 1], [2, -1], [-1, -1]]), 10, 3).tolist() == [33 + 72, 33 + 36, 33]
    cells, cut = A.verify_cells(np.array([0, 3, 0, 9, 1, 4]), 3, 7, 100, None)
    assert not cut and len(cells) == 3 and set(cells.tolist()) <= {1, 3, 4, 5} and np.all(np.diff(cells) > 0)
    again, _ = A.verify_cells(np.array([0, 3, 0, 9, 1, 4]), 3, 7, 100, None)
    assert np.array_equal(cells, again)
    cells, cut = A.verify_cells(np.array([0, 3, 0, 9, 1, 4]), 50, 7, 100, 10 ** 9)
    assert not cut and cells.tolist() == [1, 3, 4, 5]
    cells, cut = A.verify_cells(np.array([0, 3, 0, 9, 1, 4]), 4, 7, 100, 500)      # half of 500 bytes holds two grids of 100
    assert cut and len(cells) == 2


def test_writers_on_made_up_arrays(mods, tmp_path):
    A = mods["anchored"]
    barcodes, samples = ["CC-1", "AA-1", "BB-1"], ["s0", "s1", "s2", "s3"]
    A.write_anchors_tsv(str(tmp_path / "a.tsv"), barcodes, samples, np.array([5, 0, 7]), np.array([[2, 0], [0, 1], [3, -1]]), 2)
    assert (tmp_path / "a.tsv").read_text() == ("BARCODE\tN.SNP\tANCHOR.1\tANCHOR.2\tN.ENTRY\n"
                                                "BB-1\t7\ts3\t.\t16\n"
                                                "CC-1\t5\ts2\ts0\t22\n")
    c = A.write_check_tsv(str(tmp_path / "c.tsv"), ["B", "A"], ["DBL-s0-s1-0.500", "SNG-s2"], ["DBL-s0-s3-0.500", "SNG-s2"], [False, True],
                          [0.75, 1e-9], [0.5, 1e-9])
    assert c == dict(n_verified=2, n_same_call=1, n_same_pair=1)
    assert (tmp_path / "c.tsv").read_text() == (A.CHECK_HEADER + "A\tSNG-s2\tSNG-s2\t1\t1\t1e-09\t1e-09\n"
                                                "B\tDBL-s0-s1-0.500\tDBL-s0-s3-0.500\t0\t0\t0.75\t0.5\n")
    a = np.zeros((), dtype=mods["capi"].SUMMARY_DTYPE)
    a["sum_single"], a["sum_double"] = 1.0, 3.0
    assert A.prb_dbl(a) == 0.75
    (tmp_path / "x.best").write_text("BARCODE\tN.SNP\tBEST\tPRB.DBL\tPRB.SNG1\nAA-1\t5\tSNG-s1\t0.01\t0.9\n")
    assert A.read_best_columns(str(tmp_path / "x.best")) == {"AA-1": ("SNG-s1", "0.01")}


@pytest.mark.parametrize("argv", [
    ["--out", "x"], ["--pileup", "p"], ["--pileup", "p", "--out", "x", "--anchors", "0"], ["--pileup", "p", "--out", "x", "--anchors", "9"],
    ["--pileup", "p", "--out", "x", "--alpha", "0.5"], ["--pileup", "p", "--out", "x", "--alpha", "0", "1.5"],
    ["--pileup", "p", "--out", "x", "--verify", "-1"], ["--pileup", "p", "--out", "x", "--doublet-prior", "2"],
    ["--pileup", "p", "--out", "x", "--anchors", "two"],
])
def test_command_line_errors(mods, argv, capsys):
    with pytest.raises(SystemExit) as ex:
        mods["anchored"].parse_args(argv)
    assert ex.value.code == 2
    capsys.readouterr()


def test_command_line_defaults(mods):
    a = mods["anchored"].parse_args(["--pileup", "p", "--out", "x"])
    assert (a.anchors, a.alpha, a.doublet_prior, a.no_arbiter, a.verify, a.seed, a.gpu) == (2, [0.0, 0.5], 0.5, False, 0, 0, 0)
    a = mods["anchored"].parse_args(["--pileup", "p", "--out", "x", "--anchors", "8", "--alpha", "0", "0.25", "0.5", "--no-arbiter", "--verify", "7",
                                    "--seed", "3", "--min-snp", "4"])
    assert (a.anchors, a.alpha, a.no_arbiter, a.verify, a.seed, a.min_snp) == (8, [0.0, 0.25, 0.5], True, 7, 3, 4)
