"""CPU: the census uncertainty's numpy restatement (tests/census_se_ref.py) against a brute-force evaluation, the two identities,
census.covariance against the closed form and an independent statement, bound and NA handling, the calibration of the two standard
errors on committed seeds, the presence test and the reason for gap_on_support, file formats and command-line errors."""
import math

import numpy as np
import pytest

import census_ref as R
import census_se_ref as SE
from demuxlet_amd import census, synth

U = R.U
TRUE8 = np.array([.4, .25, .15, .1, .05, .03, .02, 0.0])


def tables():
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


def test_fisher_equals_brute_force_and_the_identities():
    """H of the restatement against sum_r f_r f_r' / P_r^2 in float64 and long double on 200 reads.  Bound:
    2^-52 (2 (T + V + 8) + 8) H_vu, T = reads + 2 pairs: a quotient carries the step's relative error (T + V + 8 covers it with the
    sums), it enters squared, and a term has 8 more roundings.  Identities: sum_u H_vu w_u = acc_v and w' H w = N, within the same bound
    plus the V + 1 roundings of the product with w."""
    mat, err = tables()
    rng, g, pl, _ = pool(1, V=5, S=80, B=6, n_reads=200)
    fl = R.flatten(pl)
    assert 150 < len(fl.byte) <= 200
    d, valid = R.dosage(g)
    member = np.ones(pl.n_cells, dtype=bool)
    V = 5
    for w in (np.full(5, 0.2), rng.dirichlet(np.ones(5)), np.array([0.5, 0.0, 0.3, 0.2, 0.0])):
        f = SE.fisher(fl, d, valid, member, w, mat, err, rows=2)
        s = R.step(fl, d, valid, member, w, mat, err)
        T = s.n_read + 2 * s.n_pair
        k = 2 * (T + V + 8) + 8
        assert np.array_equal(f.H, f.H.T) and (f.H >= 0).all()
        for dt in (np.float64, np.longdouble):
            Hb = SE.fisher_brute(fl, d, valid, member, w, mat, err, dtype=dt).astype(np.float64)
            ratio = float(np.max(np.abs(f.H - Hb) / (U * k * f.H)))
            print(f"H against brute force ({np.dtype(dt).name}): measured / bound {ratio:.4f}")
            assert ratio <= 1.0
        assert f.n_read == s.n_read and f.n_pair == s.n_pair and f.n_read_b.sum() == s.n_read
        assert np.all(np.abs(f.acc - s.acc) <= U * (T + V + 8) * s.acc)                 # the score rows add up to the step's acc
        Hw = f.H @ w
        assert np.all(np.abs(Hw - s.acc) <= U * (k + V + 1) * s.acc + U * (T + V + 8) * s.acc)
        assert abs(float(w @ Hw) - s.n_read) <= U * (k + 2 * V + 2 + T + V + 8) * s.n_read


@pytest.fixture(scope="module")
def fitted():
    """A pool of 8 donors fitted to a duality gap of 1e-10, its information and scores."""
    mat, err = tables()
    _, g, pl, _ = pool(2, shares=TRUE8, B=60, n_reads=6000)
    fl = R.flatten(pl)
    d, valid = R.dosage(g)
    member = np.ones(pl.n_cells, dtype=bool)
    r = R.run(fl, d, valid, member, mat, err, tol=1e-10, max_steps=20000)
    assert r["converged"]
    f = SE.fisher(fl, d, valid, member, r["w"], mat, err)
    return r, f, (fl, d, valid, member, mat, err)


def test_covariance_against_the_closed_form(fitted):
    """At a converged fit C = H_FF^-1 - w_F w_F' / N (census.covariance's docstring).  The fit's gap is 1e-10 of ~6 000 reads' LL, so
    acc_v = N holds to ~1e-7 relative on F and the two agree to that times H's condition number; this fit agrees to 4e-14; 1e-10 of the largest entry is asked."""
    r, f, _ = fitted
    c = census.covariance(f.H, r["w"], r["n_read"], f.score, f.n_read_b)
    F = c["free"]
    assert len(F) >= 6 and c["at_bound"].sum() == 8 - len(F)
    wF = r["w"][F]
    closed = np.linalg.inv(f.H[np.ix_(F, F)]) - np.outer(wF, wF) / r["n_read"]
    got = c["cov"][np.ix_(F, F)]
    rel = float(np.max(np.abs(got - closed)) / np.max(np.abs(closed)))
    print(f"covariance against the closed form: {rel:.3g} of the largest entry")
    assert rel <= 1e-10
    assert np.allclose(got.sum(axis=0), 0.0, atol=1e-12 * np.abs(got).max() * 1e4)       # shares sum to 1: rows of C sum to 0
    assert np.array_equal(c["cov"], c["cov"].T) or np.allclose(c["cov"], c["cov"].T, rtol=0, atol=1e-18)
    # the independent statement of census_se_ref (another chart of the simplex)
    se, se_r, bound = SE.covariance(f.H, r["w"], r["n_read"], f.score, f.n_read_b)
    assert np.array_equal(bound, c["at_bound"])
    assert np.allclose(se, c["se"], rtol=1e-8, atol=0) and np.allclose(se_r, c["se_robust"], rtol=1e-8, atol=0)
    assert (c["se"][F] > 0).all() and (c["se_robust"][F] > 0).all()
    assert not c["se"][c["at_bound"]].any() and not c["se_robust"][c["at_bound"]].any()


def test_bound_and_na_handling(fitted):
    r, f, _ = fitted
    w, N = r["w"], r["n_read"]
    # min_reads moves the bound: with 0.06 N every donor below 6 % is held
    c = census.covariance(f.H, w, N, f.score, f.n_read_b, min_reads=0.06 * N)
    assert c["at_bound"].tolist() == (w <= 0.06).tolist() and not c["se"][c["at_bound"]].any()
    # fewer barcodes than 2 |F|: the robust SE is NA, the model one stays
    few = np.flatnonzero(f.n_read_b > 0)[:5]
    c = census.covariance(f.H, w, N, f.score[few], f.n_read_b[few])
    F = c["free"]
    assert c["n_barcode"] == 5 and np.isnan(c["se_robust"][F]).all() and np.isfinite(c["se"][F]).all() and not np.isnan(c["se_robust"][c["at_bound"]]).any()
    # two identical donors: H is singular on the free set, both are NA there
    H2 = f.H.copy()
    H2[1, :] = H2[0, :]; H2[:, 1] = H2[:, 0]; H2[1, 1] = H2[0, 0]
    c = census.covariance(H2, w, N, f.score, f.n_read_b)
    assert np.isnan(c["se"][c["free"]]).all() and np.isnan(c["se_robust"][c["free"]]).all()
    se, se_r, _ = SE.covariance(H2, w, N, f.score, f.n_read_b)
    assert np.isnan(se[c["free"]]).all()
    # one free donor: nothing can move, SE 0; no read at all: every donor at the bound
    c = census.covariance(np.array([[4.0, 1.0], [1.0, 3.0]]), np.array([1.0, 0.0]), 10, np.zeros((3, 2)), np.array([4, 3, 3]))
    assert c["at_bound"].tolist() == [False, True] and not c["se"].any() and not c["se_robust"].any()
    c = census.covariance(np.zeros((2, 2)), np.array([0.5, 0.5]), 0, np.zeros((0, 2)), np.zeros(0))
    assert c["at_bound"].all() and not c["se"].any()
    with pytest.raises(ValueError):
        census.covariance(np.zeros((3, 3)), np.array([0.5, 0.5]), 1, np.zeros((0, 2)), np.zeros(0))


CAL = dict(S=2000, B=300, n_reads=12000, seeds=range(5000, 5024))


@pytest.fixture(scope="module")
def calibration():
    """|z| = |w^ - truth| / SE of the present donors with true share >= 0.03, over the committed seeds, for a pool whose barcodes each
    hold one donor's reads ("cells") and one whose reads are independent draws ("indep"); restatement only."""
    mat, err = tables()
    sel = TRUE8 >= 0.03
    out = {}
    for kind in ("cells", "indep"):
        zm, zr = [], []
        for seed in CAL["seeds"]:
            rng = np.random.default_rng(seed)
            raw = synth.make_raw_genotypes(rng, CAL["S"], 8)
            g = R.gt_rows(raw.alleles, 0.01)
            if kind == "cells":
                pl, _ = SE.make_cell_pool(rng, raw.alleles, TRUE8, CAL["B"], CAL["n_reads"])
            else:
                pl = R.make_pool(rng, raw.alleles, TRUE8, CAL["B"], CAL["n_reads"])
            fl = R.flatten(pl)
            d, valid = R.dosage(g)
            member = np.ones(CAL["B"], dtype=bool)
            r = R.run(fl, d, valid, member, mat, err)
            f = SE.fisher(fl, d, valid, member, r["w"], mat, err)
            c = census.covariance(f.H, r["w"], r["n_read"], f.score, f.n_read_b)
            with np.errstate(divide="ignore"):                     # (a present donor fitted at the bound has SE 0: |z| = inf, not covered)
                zm.append(np.abs(r["w"] - TRUE8)[sel] / c["se"][sel])
                zr.append(np.abs(r["w"] - TRUE8)[sel] / c["se_robust"][sel])
        out[kind] = (np.array(zm), np.array(zr))
    return out


def test_calibration(calibration):
    """Sizes chosen here for a run of about half a minute: 8 donors (.4 .25 .15 .1 .05 .03 .02 0), 2 000 SNPs, 300 barcodes, 12 000 reads
    drawn, 24 seeds; pooled over the six donors with true share >= 0.03 (144 values of |z| per pool and SE).  The thresholds: on the
    barcode-structured pool the robust SE covers (|z| < 1.96) at least 0.85 of the time and the model SE at most 0.75; on the independent
    pool both cover at least 0.85.  Measured with these seeds: cells model 0.639, robust 0.924; independent model 0.903, robust 0.910."""
    for kind, (zm, zr) in calibration.items():
        print(f"{kind}: model covers {np.mean(zm < 1.96):.3f}, robust covers {np.mean(zr < 1.96):.3f}; per donor robust "
              f"{np.mean(zr < 1.96, axis=0).round(2)}, model {np.mean(zm < 1.96, axis=0).round(2)}")
        allz = np.r_[zm.ravel(), zr.ravel()]
        assert zm.shape == (24, 6) and not np.isnan(allz).any()
        assert np.min(np.abs(allz - 1.96)) > 1e-6                  # no value sits on the threshold: the counts are not a matter of rounding
    zm, zr = calibration["cells"]
    assert np.mean(zr < 1.96) >= 0.85 and np.mean(zm < 1.96) <= 0.75
    zm, zr = calibration["indep"]
    assert np.mean(zr < 1.96) >= 0.85 and np.mean(zm < 1.96) >= 0.85


PRESENCE = dict(seed=2201, S=4000, B=300, n_reads=40000)            # the recovery pool of test_census_cpu.py / test_gpu_census.py


def presence_pool():
    rng = np.random.default_rng(PRESENCE["seed"])
    raw = synth.make_raw_genotypes(rng, PRESENCE["S"], 8)
    g = R.gt_rows(raw.alleles, 0.01)
    pl = R.make_pool(rng, raw.alleles, TRUE8, PRESENCE["B"], PRESENCE["n_reads"])
    return g, pl


def test_presence_and_the_reason_for_gap_on_support():
    """The recovery pool.  The donor with true share 0.03 is found (P < 1e-3), the absent donor is not (P > 0.1); the 0.02 donor is
    underpowered at this depth and not asserted.  A refit with a donor held at 0 converges in far fewer than max_steps passes when the gap
    runs over the support of its start; with the gap over all donors the held donor keeps acc_v > N and the refit never stops: it
    reaches max_steps (400 here, to keep the test quick: the flagged refits need a small fraction of that)."""
    mat, err = tables()
    g, pl = presence_pool()
    fl = R.flatten(pl)
    d, valid = R.dosage(g)
    member = np.ones(pl.n_cells, dtype=bool)
    full = R.run(fl, d, valid, member, mat, err)
    assert full["converged"]
    pr = SE.presence(fl, d, valid, member, mat, err, full, donors=(0, 4, 5, 7))
    print({v: (round(x["llr"], 3), f"{x['p']:.3g}", x["n_steps"], x["converged"]) for v, x in pr.items()})
    assert pr[5]["p"] < 1e-3 and pr[0]["p"] < 1e-300
    assert pr[7]["p"] > 0.1
    for v in (0, 4, 5, 7):
        assert pr[v]["converged"] == 1 and pr[v]["n_steps"] < 200
    for v in (0, 4, 5):
        assert pr[v]["w"][v] == 0.0 and abs(pr[v]["w"].sum() - 1.0) < 1e-12            # EM and SQUAREM keep the zero at zero
    # The absent donor is fitted at 6e-10, at the bound.  Left in the support of the refit without donor 4 it has acc_v / N = 1 + 3e-5,
    # grows by that factor per pass and keeps the gap at 1.24: the refits hold the donors at the bound at 0 (census.presence_test).
    y = full["w"].copy()
    y[4] = 0.0
    y /= y.sum()
    creep = SE.run(fl, d, valid, member, mat, err, w0=y, max_steps=100, gap_on_support=True)
    assert full["w"][7] > 0.0 and creep["converged"] == 0 and creep["gap"] > 1.0
    assert np.array_equal(census.presence_start(full["w"][None, :], 4, ~(full["w"][None, :] * full["n_read"] > 1.0))[0] > 0,
                          np.array([1, 1, 1, 1, 0, 1, 1, 0], dtype=bool))
    x = full["w"].copy()
    x[5] = 0.0
    x /= x.sum()
    stuck = SE.run(fl, d, valid, member, mat, err, w0=x, max_steps=400, gap_on_support=False)
    assert stuck["n_steps"] == 400 and stuck["converged"] == 0 and stuck["gap"] > 1.0
    assert 4 * pr[5]["n_steps"] < 400


def test_presence_helpers():
    assert census.presence_p(np.array([0.0]))[0] == 0.5
    assert abs(census.presence_p(np.array([1.92]))[0] - 0.025) < 5e-4                 # 2 LLR = 3.84: the 5 % point of chi-square 1, halved
    w = np.array([[0.5, 0.3, 0.2], [1.0, 0.0, 0.0]])
    x = census.presence_start(w, 0)
    assert np.allclose(x, [[0, 0.6, 0.4], [0, 0.5, 0.5]]) and np.all(np.abs(x.sum(axis=1) - 1.0) <= 1e-12) and not x[:, 0].any()
    with pytest.raises(ValueError):
        census.presence_test(lambda w0: None, np.ones((1, 1)), np.zeros(1), np.ones(1))
    # a donor at the bound everywhere is not refitted
    calls = []

    def fn(w0):
        calls.append(w0.copy())
        return dict(ll=np.array([-10.0, -7.0]), n_steps=np.array([5, 6]), converged=np.array([1, 1]))
    t = census.presence_test(fn, np.array([[0.7, 0.3, 0.0], [0.5, 0.5, 0.0]]), np.array([-8.0, -7.5]), np.array([100, 100]))
    assert len(calls) == 2 and t["llr"].tolist() == [[2.0, 2.0, 0.0], [0.0, 0.0, 0.0]] and t["p"][0, 2] == 1.0 and t["n_steps"][1, 2] == 0


def test_file_formats(tmp_path):
    names, ids = ["POOL", "SOUP"], ["smA", "smB", "smC"]
    w = np.array([[0.6, 0.4, 0.0], [0.5, 0.3, 0.2]])
    H = np.array([[50.0, 20.0, 10.0], [20.0, 60.0, 15.0], [10.0, 15.0, 70.0]])
    rng = np.random.default_rng(5)
    score = rng.uniform(5, 15, size=(12, 3))
    n_b = np.full(12, 10.0)
    covs = [census.covariance(H, w[0], 120, score, n_b), census.covariance(H, w[1], 120, score[:4], n_b[:4])]
    census.write_se_tsv(str(tmp_path / "a.census_se.tsv"), names, ids, w, covs)
    census.write_cov_tsv(str(tmp_path / "a.census_cov.tsv"), names, ids, covs)
    rows = [x.split("\t") for x in (tmp_path / "a.census_se.tsv").read_text().splitlines()]
    assert rows[0] == "GROUP SM_ID SHARE SE SE.ROBUST LO HI AT.BOUND".split() == census.SE_HEADER.rstrip("\n").split("\t") and len(rows) == 7
    assert rows[3][:3] == ["POOL", "smC", "0.000000"] and rows[3][3:] == ["0.000000", "0.000000", "0.000000", "0.000000", "1"]
    for x in rows[1:3]:
        sh, se, sr, lo, hi = map(float, x[2:7])
        assert x[7] == "0" and se > 0 and sr > 0 and abs(lo - max(sh - 1.96 * sr, 0.0)) < 2e-6 and abs(hi - min(sh + 1.96 * sr, 1.0)) < 2e-6
    for x in rows[4:]:                                                # SOUP: 4 barcodes for 3 free donors: the robust SE and the interval are NA
        assert x[0] == "SOUP" and float(x[3]) > 0 and x[4:7] == ["NA", "NA", "NA"] and x[7] == "0"
    rows = [x.split("\t") for x in (tmp_path / "a.census_cov.tsv").read_text().splitlines()]
    assert rows[0] == "GROUP SM_ID1 SM_ID2 COV COV.ROBUST".split() and len(rows) == 1 + 3 + 6
    assert [x[1:3] for x in rows[1:4]] == [["smA", "smA"], ["smA", "smB"], ["smB", "smB"]]
    assert float(rows[1][3]) == pytest.approx(covs[0]["cov"][0, 0], rel=1e-6) and float(rows[2][3]) < 0 and rows[4][4] == "NA"
    pres = dict(ll_without=np.array([[-120.5, -101.0, -100.0], [-90.0, -80.25, -80.0]]), llr=np.array([[20.5, 1.0, 0.0], [10.0, 0.25, 0.0]]),
                n_steps=np.array([[12, 9, 0], [7, 8, 5]]), converged=np.array([[1, 1, 1], [1, 0, 1]]))
    pres["p"] = census.presence_p(pres["llr"])
    census.write_presence_tsv(str(tmp_path / "a.census_presence.tsv"), names, ids, w, np.array([-100.0, -80.0]), pres)
    rows = [x.split("\t") for x in (tmp_path / "a.census_presence.tsv").read_text().splitlines()]
    assert rows[0] == "GROUP SM_ID SHARE LLK.FULL LLK.WITHOUT LLR P STEPS CONVERGED".split() and len(rows) == 7
    assert rows[1] == ["POOL", "smA", "0.600000", "-100.00000", "-120.50000", "20.50000", format(0.5 * math.erfc(math.sqrt(20.5)), ".4g"), "12", "1"]
    assert rows[3][5:] == ["0.00000", "0.5", "0", "1"] and rows[5][8] == "0"     # (write_presence_tsv prints the p it is handed)


def test_cli_flags_and_argument_errors():
    a = census.parse_args(["--pileup", "p", "--out", "x"])
    assert not a.se and not a.presence
    a = census.parse_args(["--pileup", "p", "--out", "x", "--se", "--presence"])
    assert a.se and a.presence
    with pytest.raises(SystemExit) as ei:
        census.parse_args(["--pileup", "p", "--out", "x", "--se", "3"])
    assert ei.value.code == 2
    pl = R.build_pileup(2, 3, [0], [1], [40])
    with pytest.raises(ValueError, match="at most 128"):
        census.census_run(pl, np.zeros((3, 129, 3), dtype=np.float32), [f"s{i}" for i in range(129)], None, se=True)
    with pytest.raises(ValueError, match="two samples"):
        census.census_run(pl, np.zeros((3, 1, 3), dtype=np.float32), ["a"], None, presence=True)
