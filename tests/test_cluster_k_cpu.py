"""CPU: the pure parts of choosing the number of clusters (cluster.cluster_run(auto_k=True)): the score's label
terms against a brute-force enumeration, the tie rules, the argument errors, the .kpath.tsv writer, parse_args, the pi update that keeps
merged columns out, and the numpy restatements the GPU tests lean on."""
import itertools
from math import exp

import numpy as np
import pytest

import cluster_k_ref as KR
from demuxlet_amd import cluster


def row(step, restart, k, score, **kw):
    d = dict(step=step, restart=restart, k=k, llk=-10.5, score=score, evidence=score - 3.0, dbl_score=1.0, label_term=2.0, n_sng=5, n_dbl=1,
             sizes=[3, 2], merge_k=0, merge_l=1, bf=-4.25, chosen=False)
    d.update(kw)
    return d


@pytest.mark.parametrize("n,ka", [(1, 2), (3, 2), (4, 3), (5, 1)])
def test_label_terms_are_a_distribution(n, ka):
    """Over every labelling of n barcodes (each a doublet or a singlet of one of ka clusters) exp(label term) sums to 1: the term is a
    proper prior over labellings, so scores at different K are comparable."""
    total = 0.0
    for lab in itertools.product(range(-1, ka), repeat=n):
        n_sing = [sum(x == k for x in lab) for k in range(ka)]
        n_dbl = sum(x < 0 for x in lab)
        _, _, term = cluster.path_score(np.zeros(ka), n_sing, n_dbl, 0.0, np.ones(ka))
        assert term == pytest.approx(KR.label_term(n_sing, n_dbl), abs=1e-12)
        total += exp(term)
    assert total == pytest.approx(1.0, abs=1e-12)


def test_label_term_values():
    # two barcodes, two clusters, no doublets: both in one cluster 1/3 (x P(no doublets) = 1/3), one in each 1/6 (x 1/3)
    assert exp(cluster.path_score(np.zeros(2), [2, 0], 0, 0.0, [1, 1])[2]) == pytest.approx(1 / 9)
    assert exp(cluster.path_score(np.zeros(2), [1, 1], 0, 0.0, [1, 1])[2]) == pytest.approx(1 / 18)


def test_path_score_uses_active_columns_only():
    ev = np.array([-100.0, 55.0, -200.0, -50.0])
    n = np.array([10, 99, 20, 5])
    act = np.array([1, 0, 1, 1], dtype=np.uint8)
    score, evidence, term = cluster.path_score(ev, n, 4, -30.0, act)
    assert evidence == -350.0
    assert term == pytest.approx(KR.label_term([10, 20, 5], 4), abs=1e-12)
    assert score == pytest.approx(-350.0 - 30.0 + term, abs=1e-12)
    assert score == pytest.approx(KR.path_score(ev, n, 4, -30.0, act), abs=1e-9)


def test_best_active_pair_ties_and_inactive():
    K = 4                                                  # pairs: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
    bf = np.array([-5.0, 7.0, 7.0, -1.0, 7.0, 9.0])
    assert cluster.best_active_pair(bf, np.ones(K)) == (2, 3, 9.0)
    assert cluster.best_active_pair(bf, [1, 1, 1, 0]) == (0, 2, 7.0)          # (2, 3) is out; the lowest of the tied pairs
    assert cluster.best_active_pair(bf, [0, 1, 1, 1]) == (2, 3, 9.0)
    assert cluster.best_active_pair(bf, [1, 1, 0, 0]) == (0, 1, -5.0)
    # an emptied column: BF exactly 0 against everyone, above the negative scores of distinct donors; the lowest pair first
    assert cluster.best_active_pair(np.array([-3.0, 0.0, -8.0, 0.0, -2.0, 0.0]), np.ones(K)) == (0, 2, 0.0)
    with pytest.raises(ValueError):
        cluster.best_active_pair(bf, [0, 0, 1, 0])


def test_path_winner_ties():
    rows = [row(0, 0, 4, -10.0), row(0, 1, 4, -7.0), row(1, 0, 3, -7.0), row(1, 1, 3, -7.0), row(2, 0, 2, -9.0), row(2, 1, 2, -8.0)]
    assert cluster.path_winner(rows) == 2                  # the smaller K, then the lower restart
    assert cluster.path_winner(rows[:2]) == 1
    assert cluster.path_winner([row(0, 0, 4, -7.0), row(0, 1, 4, -7.0)]) == 0
    assert cluster.path_winner(rows[::-1]) == len(rows) - 1 - 2


def test_auto_k_argument_errors():
    cluster.check_auto_k_args(8, 2, False)
    cluster.check_auto_k_args(4, 4, False)
    cluster.check_auto_k_args(64, 2, False)
    for K, k_min, sm in [(8, 1, False), (8, 9, False), (65, 2, False), (8, 2, True), (8, 0, False)]:
        with pytest.raises(ValueError):
            cluster.check_auto_k_args(K, k_min, sm)


def test_cluster_run_checks_auto_k_before_any_device_work():
    from demuxlet_amd import engine
    z = np.zeros(0, dtype=np.int64)
    pl = engine.HostPileup(10, 5, np.arange(11, dtype=np.int64), np.arange(11, dtype=np.int64), np.zeros(10, dtype=np.int32),
                           np.ones(10, dtype=np.uint8), np.zeros(10, dtype=np.uint8), z, z, z)
    names = [f"b{i}" for i in range(10)]
    with pytest.raises(ValueError, match="split-merge"):
        cluster.cluster_run(pl, 4, "/nonexistent/x", barcodes=names, auto_k=True, split_merge=True)
    with pytest.raises(ValueError, match="k-min"):
        cluster.cluster_run(pl, 4, "/nonexistent/x", barcodes=names, auto_k=True, k_min=5)
    with pytest.raises(ValueError, match="k-min"):
        cluster.cluster_run(pl, 4, "/nonexistent/x", barcodes=names, auto_k=True, k_min=1)


def test_kpath_writer(tmp_path):
    rows = [row(0, 0, 3, -100.123456789, sizes=[4, 0, 2], chosen=False), row(0, 1, 3, -90.5, merge_k=1, merge_l=2, bf=0.0),
            row(1, 0, 2, -80.25, merge_k=-1, merge_l=-1, bf=float("nan"), chosen=True)]
    p = tmp_path / "x.kpath.tsv"
    cluster.write_kpath_tsv(str(p), rows)
    lines = p.read_text().splitlines()
    assert lines[0] + "\n" == cluster.KPATH_HEADER
    head = lines[0].split("\t")
    assert head == "STEP RESTART K LLK SCORE EVIDENCE DBL.SCORE LABEL.TERM N.SNG N.DBL SIZES MERGE_K MERGE_L BF CHOSEN".split()
    cells = [dict(zip(head, ln.split("\t"))) for ln in lines[1:]]
    assert len(cells) == 3 and all(len(ln.split("\t")) == len(head) for ln in lines[1:])
    assert cells[0]["SCORE"] == "-100.123457" and cells[0]["SIZES"] == "4,0,2" and cells[0]["K"] == "3" and cells[0]["CHOSEN"] == "0"
    assert cells[1]["MERGE_K"] == "1" and cells[1]["MERGE_L"] == "2" and cells[1]["BF"] == "0.000000"
    assert cells[2]["BF"] == "NA" and cells[2]["MERGE_K"] == "-1" and cells[2]["CHOSEN"] == "1"
    assert [c["CHOSEN"] for c in cells].count("1") == 1


def test_parse_args():
    base = ["--pileup", "x", "--out", "o", "--n-clusters", "8"]
    a = cluster.parse_args(base)
    assert a.auto_k is False and a.k_min is None
    a = cluster.parse_args(base + ["--auto-k"])
    assert a.auto_k is True and a.k_min == 2
    a = cluster.parse_args(base + ["--auto-k", "--k-min", "3", "--em-doublets"])
    assert a.k_min == 3 and a.em_doublets
    for bad in (["--k-min", "3"], ["--auto-k", "--k-min", "1"], ["--auto-k", "--k-min", "9"], ["--auto-k", "--split-merge"]):
        with pytest.raises(SystemExit):
            cluster.parse_args(base + bad)
    with pytest.raises(SystemExit):
        cluster.parse_args(["--pileup", "x", "--out", "o", "--n-clusters", "65", "--restarts", "1", "--auto-k"])


def test_active_pi_update_keeps_merged_columns_out():
    act = np.array([[1, 0, 1, 1], [1, 1, 1, 1], [0, 0, 1, 0]], dtype=np.uint8)
    cs = np.array([[30.0, 1e-300, 10.0, 0.0], [1.0, 2.0, 3.0, 4.0], [0.0, 5.0, 0.0, 0.0]])
    lp = cluster.update_log_pi_active(cs.reshape(-1), act)
    assert lp.shape == (3, 4)
    assert np.isneginf(lp[act == 0]).all() and np.isfinite(lp[act == 1]).all()
    pi = np.exp(lp)
    assert np.allclose(pi.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    assert (pi[act == 1] >= cluster.PI_FLOOR * (1 - 1e-5)).all()           # an active column with no mass keeps the floor
    assert pi[0, 0] == pytest.approx(0.75, rel=1e-5) and pi[0, 2] == pytest.approx(0.25, rel=1e-5)
    assert pi[2, 2] == 1.0                                                  # the inactive column's sum is ignored
    # every column active: today's update, bit for bit
    assert np.array_equal(cluster.update_log_pi_active(cs[1], np.ones((1, 4))), cluster.update_log_pi(cs[1], 1, 4))
    # the existing update would revive a merged column
    assert np.isfinite(cluster.update_log_pi(cs[0], 1, 4)).all()


def test_reference_hard_labels_and_merge():
    w = np.array([[0.2, 0.5, 0.3, 0.0], [0.4, 0.1, 0.4, 0.1], [0.0, 0.9, 0.05, 0.05], [0.25, 0.25, 0.25, 0.25]])
    act = np.array([[1, 0, 1, 1]])
    mask = np.array([1, 1, 1, 0], dtype=bool)
    dm = np.array([[0.0], [0.1], [0.7], [0.9]])
    lld = np.zeros((4, 1, 6))
    lld[2, 0] = [9.0, -1.0, -3.0, 5.0, 5.0, -3.0]          # active pairs: (0,2) p=1, (0,3) p=2, (2,3) p=5; the tie -3 / -3 loses to -1
    label, n_sing, n_dbl, score, hot = KR.hard(w, act, 1, 4, mask, dm, lld)
    assert label[:, 0].tolist() == [2, 0, -3, -1]         # barcode 1: the tie 0.4 / 0.4 goes to the lower column
    assert n_sing.tolist() == [[1, 0, 1, 0]] and n_dbl.tolist() == [1] and score.tolist() == [-1.0]
    assert hot.tolist() == [[0, 0, 1, 0], [1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    m = KR.merge_columns(w, 1, 4, [3], [0])
    assert np.array_equal(m[:, 0], w[:, 0] + w[:, 3]) and not m[:, 3].any() and np.array_equal(m[:, 1:3], w[:, 1:3])
    assert np.array_equal(KR.merge_columns(w, 1, 4, [-1], [0]), w)


def test_reference_evidence_skips_uncovered_snps():
    rng = np.random.default_rng(3)
    S, C = 300, 2
    LL = -rng.random((S, C, 3)) * 5
    W = rng.random((S, C))
    W[:, 1] = 0.0
    W[::3, 0] = 0.0
    q = cluster.hwe_prior(rng.integers(0, 9, S), rng.integers(0, 9, S))
    ev, nc = KR.evidence(LL, W, q, 1e-3, 1, C)
    assert ev[0, 1] == 0.0 and nc[0, 1] == 0 and nc[0, 0] == S - len(range(0, S, 3))
    a = q.astype(np.float64) + 1e-3
    lp = np.log(a / a.sum(axis=1, keepdims=True))
    direct = sum(np.log(np.exp(lp[i] + LL[i, 0]).sum()) for i in range(S) if W[i, 0] > 0)
    assert ev[0, 0] == pytest.approx(direct, rel=1e-12)
