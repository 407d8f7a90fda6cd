"""CPU: the doublet-aware EM without a GPU — the float64 restatement of the doublet E-step
(tests/cluster_dbl_ref.py) and its limits, the pair order, the delta update and its clipping, --em-doublets parsing and the .em.tsv
format with and without the flag."""
import numpy as np
import pytest

import cluster_dbl_ref as D
from demuxlet_amd import cluster


def test_pair_order_is_lexicographic():
    for K in (2, 3, 5, 12, 40):
        p = cluster.pair_index(K)
        assert p.shape == (K * (K - 1) // 2, 2)
        assert np.array_equal(p, D.pairs(K))
        assert (p[:, 0] < p[:, 1]).all()
        assert [tuple(x) for x in p] == sorted(tuple(x) for x in p)
    assert [tuple(x) for x in cluster.pair_index(4)] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def test_priors_are_a_distribution():
    rng = np.random.default_rng(1)
    R, K = 3, 6
    log_pi = np.log(rng.dirichlet(np.ones(K), size=R))
    delta = np.array([0.1, 0.25, 0.001])
    lps, lpd = D.log_priors(log_pi, np.log(delta))
    assert np.allclose(np.exp(lps).sum(axis=1), 1.0 - delta, rtol=1e-14)
    assert np.allclose(np.exp(lpd).sum(axis=1), delta, rtol=1e-13)
    lps0, lpd0 = D.log_priors(log_pi, np.full(R, -np.inf))
    assert np.array_equal(lps0, log_pi) and np.isneginf(lpd0).all()


def random_case(rng, B, R, K, spread=30.0):
    llks = rng.normal(-500.0, spread, size=(B, R * K))
    lld = rng.normal(-500.0, spread, size=(B, R, K * (K - 1) // 2))
    log_pi = np.log(rng.dirichlet(np.ones(K), size=R))
    return llks, lld, log_pi


@pytest.mark.parametrize("T", [1.0, 2.5])
def test_restated_estep_masses(T):
    rng = np.random.default_rng(2)
    B, R, K = 200, 3, 5
    llks, lld, log_pi = random_case(rng, B, R, K)
    mask = rng.random(B) < 0.8
    w, dm, ll, cs, dbl = D.estep(llks, lld, log_pi, np.log([0.1, 0.2, 0.3]), T, mask)
    tot = w.reshape(B, R, K).sum(axis=2) + dm
    assert np.allclose(tot[mask], 1.0, rtol=1e-13) and not tot[~mask].any()
    assert np.allclose(cs, w.sum(axis=0)) and np.allclose(dbl, dm.sum(axis=0))
    assert np.isclose(cs.reshape(R, K).sum(axis=1) + dbl, mask.sum(), rtol=1e-12).all()
    assert np.isfinite(ll).all()


def test_restated_estep_without_doublets_is_the_plain_one():
    """delta -> 0 (log_delta = -inf): the doublet components vanish and the restated E-step is section 13's."""
    rng = np.random.default_rng(3)
    B, R, K = 300, 4, 6
    llks, lld, log_pi = random_case(rng, B, R, K)
    mask = rng.random(B) < 0.7
    for T, mk in ((1.0, None), (1.7, mask)):
        w, dm, ll, cs, dbl = D.estep(llks, lld, log_pi, np.full(R, -np.inf), T, mk)
        pw, pll, pcs = D.estep_plain(llks, log_pi, T, mk)
        assert not dm.any() and not dbl.any()
        assert np.allclose(w, pw, rtol=1e-14, atol=0) and np.allclose(ll, pll, rtol=1e-14) and np.allclose(cs, pcs, rtol=1e-14)
    # and as delta shrinks the results approach it (doublet likelihoods no better than the singlets')
    w1, _, ll1, _, _ = D.estep(llks, lld - 200.0, log_pi, np.full(R, np.log(1e-12)))
    pw, pll, _ = D.estep_plain(llks, log_pi)
    assert np.abs(w1 - pw).max() < 1e-9 and np.allclose(ll1, pll, rtol=1e-12)


def test_restated_estep_sends_a_doublet_to_the_doublet_component():
    """A barcode whose doublet likelihood for pair (1, 3) clearly beats every singlet puts its mass there and nothing in clusters 1, 3."""
    R, K = 1, 4
    llks = np.full((1, K), -1000.0)
    lld = np.full((1, R, 6), -1100.0)
    lld[0, 0, list(map(tuple, D.pairs(K))).index((1, 3))] = -900.0
    w, dm, ll, cs, dbl = D.estep(llks, lld, np.full((R, K), -np.log(K)), np.log([0.1]))
    assert dm[0, 0] > 1 - 1e-12 and w.max() < 1e-12
    assert np.isclose(ll[0], -900.0 + np.log(0.1 * 2 / 16 / (1 - 4 / 16)), rtol=1e-12)


def test_delta_update_and_clipping():
    d = cluster.update_delta(np.array([25.0, 0.0, 90.0, 1e-2, 50.0]), 100)
    assert np.allclose(d, [0.25, cluster.DELTA_MIN, cluster.DELTA_MAX, 1e-3, 0.5])
    assert cluster.DELTA0 == 0.1 and cluster.DELTA_MIN == 1e-3 and cluster.DELTA_MAX == 0.5
    assert np.allclose(cluster.update_delta(np.array([3.0]), 0), [cluster.DELTA_MAX])     # an empty mask does not divide by zero
    # the update is the share of the restated E-step's doublet mass
    rng = np.random.default_rng(4)
    llks, lld, log_pi = random_case(rng, 500, 2, 3, spread=2.0)
    _, dm, _, _, dbl = D.estep(llks, lld, log_pi, np.log([0.2, 0.2]))
    assert np.allclose(cluster.update_delta(dbl, 500), np.clip(dm.mean(axis=0), 1e-3, 0.5))


def test_parse_em_doublets():
    a = cluster.parse_args(["--pileup", "p", "--n-clusters", "4", "--out", "o"])
    assert a.em_doublets is False
    a = cluster.parse_args(["--pileup", "p", "--n-clusters", "4", "--out", "o", "--em-doublets", "--restarts", "3"])
    assert a.em_doublets is True and a.restarts == 3
    with pytest.raises(SystemExit):
        cluster.parse_args(["--pileup", "p", "--n-clusters", "1", "--out", "o", "--em-doublets"])
    with pytest.raises(SystemExit):
        cluster.parse_args(["--pileup", "p", "--n-clusters", "4", "--out", "o", "--em-doublets=1"])


def test_em_tsv_with_and_without_doublets(tmp_path):
    rows = [(1, 0, -1234.5, [0.25, 0.75]), (1, 1, -1200.0, [0.5, 0.5])]
    cluster.write_em_tsv(str(tmp_path / "a.em.tsv"), rows)
    assert (tmp_path / "a.em.tsv").read_text() == "ITER\tRESTART\tLLK\tPI\n1\t0\t-1234.500000\t0.25,0.75\n1\t1\t-1200.000000\t0.5,0.5\n"
    drows = [r + (d,) for r, d in zip(rows, (0.1, 0.2345678))]
    cluster.write_em_tsv(str(tmp_path / "b.em.tsv"), drows, doublets=True)
    assert (tmp_path / "b.em.tsv").read_text() == \
        "ITER\tRESTART\tLLK\tPI\tDBL\n1\t0\t-1234.500000\t0.25,0.75\t0.1\n1\t1\t-1200.000000\t0.5,0.5\t0.234568\n"
    # without the flag, rows that carry a delta still give today's format
    cluster.write_em_tsv(str(tmp_path / "c.em.tsv"), drows)
    assert (tmp_path / "c.em.tsv").read_bytes() == (tmp_path / "a.em.tsv").read_bytes()
