"""CPU: the donor-share census' numpy restatement (tests/census_ref.py) against a brute-force evaluation, the properties the engine's
driver relies on (EM never lowers LL, the duality gap bounds the LL still to be gained, SQUAREM reaches the plain run's LL), and
census.py's group handling and command-line errors."""
import math

import numpy as np
import pytest

import census_ref as R
from demuxlet_amd import census, synth

TRUE8 = np.array([.4, .25, .15, .1, .05, .03, .02, 0.0])


def tables():
    """Phred tables for the restatement, which takes whatever tables it is handed: err = 10^(-q/10), capped at 0.75."""
    q = np.arange(256)
    err = np.minimum(10.0 ** (-q / 10.0), 0.75)
    return 1.0 - err, err


def pool(seed, V=8, S=600, B=40, n_reads=3000, shares=None):
    rng = np.random.default_rng(seed)
    raw = synth.make_raw_genotypes(rng, S, V)
    g = R.gt_rows(raw.alleles, 0.01)
    shares = rng.dirichlet(np.ones(V)) if shares is None else shares
    pl = R.make_pool(rng, raw.alleles, shares, B, n_reads)
    return rng, g, pl, shares


def test_step_equals_brute_force():
    mat, err = tables()
    rng, g, pl, _ = pool(1, V=5, S=80, B=6, n_reads=200)
    fl = R.flatten(pl)
    assert 150 < len(fl.byte) <= 200
    d, valid = R.dosage(g)
    member = np.ones(pl.n_cells, dtype=bool)
    for w in (np.full(5, 0.2), rng.dirichlet(np.ones(5)), np.array([0.5, 0.0, 0.3, 0.2, 0.0])):
        s = R.step(fl, d, valid, member, w, mat, err)
        acc64, ll64 = R.step_brute(fl, d, valid, member, w, mat, err)
        accl, lll = R.step_brute(fl, d, valid, member, w, mat, err, dtype=np.longdouble)
        T = s.n_read + 2 * s.n_pair
        for acc, ll in ((acc64, ll64), (accl, lll)):
            assert np.all(np.abs(s.acc - acc.astype(np.float64)) <= R.U * (T + 5 + 8) * s.acc)
            assert abs(s.ll - float(ll)) <= R.U * (T + 3) * s.abs_log
        assert abs(float((w * s.acc).sum()) - s.n_read) <= R.U * (T + 16) * s.n_read       # sum_v w_v acc_v = N
        assert s.gap >= -R.U * (T + 16) * s.n_read


def test_dosage_and_invalid_snps():
    g = np.zeros((3, 2, 3), dtype=np.float32)
    g[0] = [[1, 0, 0], [0, 0, 1]]
    g[1] = [[0.25, 0.5, 0.25], [0, 0, 0]]           # one all-zero row: the SNP is invalid
    g[2] = [[0, 2, 0], [0.5, 0, 1.5]]               # rows need not sum to 1
    d, valid = R.dosage(g)
    assert valid.tolist() == [True, False, True]
    assert d[0].tolist() == [0.0, 1.0] and d[1, 1] == 0.0 and d[2].tolist() == [0.5, 0.75]
    d2, v2 = census.dosage(g)
    assert np.array_equal(d, d2) and np.array_equal(valid, v2)
    a = census.ambient_profile(np.array([0.25, 0.75]), g)
    assert a[0] == 0.75 and np.isnan(a[1]) and a[2] == 0.25 * 0.5 + 0.75 * 0.75


def test_plain_em_never_lowers_ll_and_gap_bounds_the_rest():
    mat, err = tables()
    _, g, pl, _ = pool(2, shares=TRUE8)
    fl = R.flatten(pl)
    d, valid = R.dosage(g)
    member = np.ones(pl.n_cells, dtype=bool)
    long_path = []
    w_long = R.run(fl, d, valid, member, mat, err, tol=1e-10, max_steps=20000, accelerate=False, path=long_path)
    assert w_long["converged"] and w_long["gap"] <= 1e-10
    lls = np.array([s.ll for _, s in long_path])
    slack = R.U * (fl.nrd.sum() + 3) * long_path[0][1].abs_log
    assert np.all(np.diff(lls) >= -slack)
    for _, s in long_path:
        assert w_long["ll"] - s.ll <= s.gap + slack
    # the same bound along a SQUAREM path
    sq_path = []
    sq = R.run(fl, d, valid, member, mat, err, path=sq_path)
    for _, s in sq_path:
        assert w_long["ll"] - s.ll <= s.gap + slack
    assert sq["converged"] and sq["gap"] <= 1e-4
    assert abs(sq["ll"] - w_long["ll"]) <= 1e-4 + slack
    assert sq["n_steps"] < len([1 for _, s in long_path if s.gap > 1e-4]) + 1      # fewer passes than plain EM needs for the same gap
    assert abs(sq["w"].sum() - 1.0) < 1e-12 and (sq["w"] >= 0).all()


def test_recovery_seed_on_cpu():
    """The pool of test_gpu_census.py's recovery test: 8 donors, 4 000 SNPs, 40 000 reads drawn, GT rows with error 0.01, base qualities
    10-40.  The committed seed's own error has to be below 0.02 for the GPU test's 0.03 to be a sound threshold."""
    mat, err = tables()
    rng = np.random.default_rng(2201)
    raw = synth.make_raw_genotypes(rng, 4000, 8)
    g = R.gt_rows(raw.alleles, 0.01)
    pl = R.make_pool(rng, raw.alleles, TRUE8, 300, 40000)
    fl = R.flatten(pl)
    d, valid = R.dosage(g)
    r = R.run(fl, d, valid, np.ones(300, dtype=bool), mat, err)
    e = float(np.abs(r["w"] - TRUE8).max())
    print(f"recovery: max |w - truth| = {e:.4f}, absent donor {r['w'][7]:.4f}, steps {r['n_steps']}")
    assert r["converged"] and e < 0.02 and r["w"][7] < 0.01


def test_max_steps_and_empty_group():
    mat, err = tables()
    _, g, pl, _ = pool(3)
    fl = R.flatten(pl)
    d, valid = R.dosage(g)
    r = R.run(fl, d, valid, np.ones(pl.n_cells, dtype=bool), mat, err, max_steps=3)
    assert r["n_steps"] == 3 and r["converged"] == 0
    w0 = np.array([0.5, 0.5, 0, 0, 0, 0, 0, 0.0])
    r = R.run(fl, d, valid, np.zeros(pl.n_cells, dtype=bool), mat, err, w0=w0)
    assert r["n_steps"] == 1 and r["converged"] == 1 and r["ll"] == 0.0 and r["n_read"] == 0 and np.array_equal(r["w"], w0)


def test_extrapolate_stays_on_the_simplex():
    rng = np.random.default_rng(4)
    for _ in range(200):
        w0 = rng.dirichlet(np.ones(6) * 0.3)
        w1 = rng.dirichlet(np.ones(6) * 0.3)
        w2 = rng.dirichlet(np.ones(6) * 0.3)
        x = R.extrapolate(w0, w1, w2)
        assert (x >= 0).all() and abs(x.sum() - 1.0) < 1e-12
    w = np.array([0.2, 0.8])
    assert np.array_equal(R.extrapolate(w, w, w), w)           # a fixed point: r = u = 0, steplength -1, the second iterate


def test_read_groups(tmp_path):
    bcs = ["AAA-1", "CCC-1", "GGG-1", "TTT-1"]
    p = tmp_path / "g.tsv"
    p.write_text("# comment\nGGG-1\tsoup\nAAA-1\tcells\n\nTTT-1\tsoup\n")
    group, names = census.read_groups(str(p), bcs)
    assert names == ["soup", "cells"] and group.tolist() == [1, -1, 0, 0] and group.dtype == np.int32
    for bad in ("AAA-1 cells\n", "NNN-1\tx\n", "AAA-1\tx\nAAA-1\ty\n", "AAA-1\t\n", "# nothing\n"):
        p.write_text(bad)
        with pytest.raises(ValueError):
            census.read_groups(str(p), bcs)


def test_split_by_reads():
    group, names = census.split_by_reads(np.array([0, 5, 6, 100]), 5)
    assert names == ["EMPTY", "CELLS"] and group.tolist() == [0, 0, 1, 1] and group.dtype == np.int32
    with pytest.raises(ValueError):
        census.split_by_reads(np.array([1]), -1)


@pytest.mark.parametrize("argv", [
    ["--out", "x"],                                                       # no --pileup
    ["--pileup", "p"],                                                    # no --out
    ["--pileup", "p", "--out", "x", "--groups", "g", "--max-reads", "3"],
    ["--pileup", "p", "--out", "x", "--max-reads", "-1"],
    ["--pileup", "p", "--out", "x", "--tol", "0"],
    ["--pileup", "p", "--out", "x", "--tol", "nan"],
    ["--pileup", "p", "--out", "x", "--max-steps", "0"],
    ["--pileup", "p", "--out", "x", "--gpu", "-1"],
    ["--pileup", "p", "--out", "x", "--accel"],
])
def test_cli_argument_errors(argv, capsys):
    with pytest.raises(SystemExit) as ei:
        census.parse_args(argv)
    assert ei.value.code == 2
    capsys.readouterr()


def test_cli_defaults():
    a = census.parse_args(["--pileup", "p", "--out", "x"])
    assert a.tol == 1e-4 and a.max_steps == 2000 and not a.no_accel and a.groups is None and a.max_reads is None and a.gpu == 0
    assert census.parse_args(["--pileup", "p", "--out", "x", "--no-accel", "--max-reads", "0"]).max_reads == 0


def test_census_run_argument_errors():
    pl = R.build_pileup(2, 3, [0], [1], [40])
    g = np.zeros((3, 2, 3), dtype=np.float32)
    with pytest.raises(ValueError):
        census.census_run(pl, g, ["a", "b"], None, groups=(np.zeros(2), ["x"]), max_reads=1)
    with pytest.raises(ValueError):
        census.census_run(pl, g[:2], ["a", "b"], None)
    with pytest.raises(ValueError):
        census.census_run(pl, g, ["a", "b"], None, groups="somefile")                 # a HostPileup without barcodes=
    with pytest.raises(ValueError):
        census.census_run(pl, g, ["a", "b"], None, groups=(np.array([0, 2]), ["x", "y"]))
    with pytest.raises(ValueError):
        census.ambient_profile(np.ones(3) / 3, g)
    assert math.isnan(census.ambient_profile(np.array([0.5, 0.5]), g)[0])
