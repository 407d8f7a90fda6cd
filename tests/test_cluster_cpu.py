"""CPU: the genotype-free clustering driver (demuxlet_amd/cluster.py) without a GPU — option parsing and its error paths, the HWE prior,
the seeded initialisation, the EM bookkeeping, the .em.tsv / .clust.tsv / .match.tsv writers and the label-matching helper."""
import numpy as np
import pytest

from demuxlet_amd import cluster, engine, refine


def test_parse_args_defaults_and_options():
    a = cluster.parse_args(["--pileup", "x.pileup.txt", "--n-clusters", "6", "--out", "o"])
    assert (a.n_clusters, a.restarts, a.seed, a.max_iter, a.tol, a.floor, a.min_snp, a.alpha, a.rounds, a.match, a.fast, a.gpu) == \
        (6, 16, 0, 50, 1e-7, 1e-3, 0, [0.0, 0.5], 1, False, False, 0)
    a = cluster.parse_args(["--pileup", "p", "--n-clusters", "3", "--out", "o", "--restarts", "2", "--seed", "9", "--max-iter", "7", "--tol", "1e-5",
                            "--floor", "0.01", "--min-snp", "5", "--alpha", "0", "0.25", "0.5", "--rounds", "0", "--match", "--fast", "--gpu", "1"])
    assert (a.restarts, a.seed, a.max_iter, a.tol, a.floor, a.min_snp, a.alpha, a.rounds, a.match, a.fast, a.gpu) == \
        (2, 9, 7, 1e-5, 0.01, 5, [0.0, 0.25, 0.5], 0, True, True, 1)


@pytest.mark.parametrize("argv", [
    ["--pileup", "p", "--n-clusters", "1", "--out", "o"],                          # K < 2
    ["--pileup", "p", "--n-clusters", "2048", "--out", "o", "--restarts", "2"],     # R * K > the engine's limit
    ["--pileup", "p", "--n-clusters", "300", "--out", "o"],                         # ... with the default 16 restarts
    ["--pileup", "p", "--n-clusters", "4", "--out", "o", "--restarts", "0"],
    ["--n-clusters", "4", "--out", "o"],                                            # no pileup
])
def test_parse_args_refuses(argv):
    with pytest.raises(SystemExit):
        cluster.parse_args(argv)


def test_check_args_error_paths():
    cluster.check_args(4, 4, 50, 1e-7, 1e-3, 100, 1000)
    with pytest.raises(ValueError, match="at least 2"):
        cluster.check_args(1, 4, 50, 1e-7, 1e-3, 100, 1000)
    with pytest.raises(ValueError, match="at most 4094"):
        cluster.check_args(1024, 4, 50, 1e-7, 1e-3, 100_000, 10**6)
    with pytest.raises(ValueError, match="empty pileup"):
        cluster.check_args(4, 4, 50, 1e-7, 1e-3, 100, 0)
    with pytest.raises(ValueError, match="empty pileup"):
        cluster.check_args(4, 4, 50, 1e-7, 1e-3, 3, 10)
    with pytest.raises(ValueError):
        cluster.check_args(4, 4, 0, 1e-7, 1e-3, 100, 10)


def test_cluster_run_refuses_before_device_work(tmp_path):
    """The checks run before any engine exists, so they need no GPU."""
    z = np.zeros(0, dtype=np.int32)
    empty = engine.HostPileup(5, 10, np.zeros(6, dtype=np.int64), np.zeros(6, dtype=np.int64), z, np.zeros(0, dtype=np.uint8),
                              np.zeros(0, dtype=np.uint8), np.zeros(5, np.int32), np.zeros(5, np.int32), np.zeros(5, np.int32))
    with pytest.raises(ValueError, match="empty pileup"):
        cluster.cluster_run(empty, 2, str(tmp_path / "o"), barcodes=[f"b{i}" for i in range(5)])
    with pytest.raises(ValueError, match="at most"):
        cluster.cluster_run(empty, 1000, str(tmp_path / "o"), restarts=5, barcodes=[f"b{i}" for i in range(5)])
    with pytest.raises(ValueError, match="barcodes="):
        cluster.cluster_run(empty, 2, str(tmp_path / "o"))
    assert not list(tmp_path.iterdir())


def test_main_refuses_empty_pileup_dump(tmp_path):
    d = refine.PileupDump(["s0"], [(1, 100, "A", "G")], np.full((1, 1, 3), 1 / 3, dtype=np.float32), ["AAAA", "CCCC"],
                          engine.HostPileup(2, 1, np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int32),
                                            np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), np.zeros(2, np.int32),
                                            np.zeros(2, np.int32), np.zeros(2, np.int32)))
    p = tmp_path / "x.pileup.txt"
    refine.write_pileup_txt(str(p), d)
    with pytest.raises(ValueError, match="empty pileup"):
        cluster.main(["--pileup", str(p), "--n-clusters", "2", "--out", str(tmp_path / "o")])
    with pytest.raises(ValueError, match="empty pileup"):
        cluster.main(["--pileup", str(p), "--n-clusters", "2", "--out", str(tmp_path / "o"), "--match"])
    assert sorted(x.name for x in tmp_path.iterdir()) == ["x.pileup.txt"]


def test_hwe_prior():
    n_ref = np.array([0, 10, 3, 0])
    n_alt = np.array([0, 0, 3, 8])
    q = cluster.hwe_prior(n_ref, n_alt)
    assert q.dtype == np.float32 and q.shape == (4, 3)
    p = (n_alt + 1.0) / (n_ref + n_alt + 2.0)
    want = np.stack([(1 - p) ** 2, 2 * p * (1 - p), p ** 2], axis=1).astype(np.float32)
    assert np.array_equal(q, want)
    assert np.allclose(q[0], [0.25, 0.5, 0.25]) and np.allclose(q[2], [0.25, 0.5, 0.25])
    assert np.allclose(q.sum(axis=1), 1.0, atol=1e-6)
    assert q[1, 0] > 0.8 and q[3, 2] > 0.6


def test_initial_labels_reproducible():
    a = cluster.initial_labels(7, 3, 500, 5)
    b = cluster.initial_labels(7, 3, 500, 5)
    c = cluster.initial_labels(8, 3, 500, 5)
    assert a.shape == (3, 500) and a.dtype == np.int32
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert not np.array_equal(a[0], a[1])                      # each restart its own draw
    assert a.min() == 0 and a.max() == 4


def test_one_hot_weights_and_mask():
    lab = np.array([[0, 1, 2, 1], [2, 2, 0, 1]], dtype=np.int32)
    w = cluster.one_hot_weights(lab, 3, mask=np.array([1, 1, 0, 1], dtype=bool))
    assert w.shape == (4, 6)
    assert np.array_equal(w.sum(axis=1), [2, 2, 0, 2])
    assert w[0, 0] == 1 and w[0, 3 + 2] == 1 and w[3, 1] == 1 and w[3, 3 + 1] == 1


def test_update_log_pi_and_convergence():
    lp = cluster.update_log_pi(np.array([3.0, 1.0, 0.0, 2.0, 2.0, 0.0]), 2, 3)
    pi = np.exp(lp)
    assert np.allclose(pi.sum(axis=1), 1.0)
    assert np.allclose(pi[0, :2], [0.75, 0.25], atol=1e-5) and pi[0, 2] > 0 and pi[1, 2] > 0
    assert not cluster.converged(None, np.array([-10.0]), 1e-7)
    assert cluster.converged(np.array([-1e6, -2e6]), np.array([-1e6 + 0.01, -2e6]), 1e-7)
    assert not cluster.converged(np.array([-1e6, -2e6]), np.array([-1e6 + 1.0, -2e6]), 1e-7)
    assert cluster.best_restart(np.array([-5.0, -3.0, -3.0])) == 1


def test_write_em_tsv(tmp_path):
    p = tmp_path / "o.em.tsv"
    cluster.write_em_tsv(str(p), [(1, 0, -123.456789, [0.5, 0.5]), (1, 1, -120.0, [0.25, 0.75])])
    lines = p.read_text().splitlines()
    assert lines[0] == "ITER\tRESTART\tLLK\tPI"
    assert lines[1] == "1\t0\t-123.456789\t0.5,0.5"
    assert lines[2] == "1\t1\t-120.000000\t0.25,0.75"


def test_clust_tsv_uses_refined_format(tmp_path):
    S, K = 3, 2
    ll = np.arange(S * K * 3, dtype=np.float64).reshape(S, K, 3) * -0.5
    n_cell = np.array([[1, 0], [0, 0], [2, 3]], dtype=np.int32)
    gp = np.full((S, K, 3), 1 / 3, dtype=np.float32)
    p = tmp_path / "o.clust.tsv"
    refine.write_refined_tsv(str(p), None, cluster.cluster_ids(K), ll, n_cell, n_cell, n_cell * 0, gp)
    lines = p.read_text().splitlines()
    assert lines[0] + "\n" == refine.REFINED_HEADER
    assert [ln.split("\t")[4] for ln in lines[1:]] == ["CLUST0", "CLUST0", "CLUST1"]


def test_match_table_and_writer(tmp_path):
    llks = np.array([[-1.0, -9.0, -5.0], [-2.0, -8.0, -5.0], [-9.0, -1.0, -5.0], [-3.0, -3.0, -3.0]])
    called = np.array([0, 0, 1, -1])
    n, s = cluster.match_table(llks, called, 3)
    assert list(n) == [2, 1, 0]
    assert np.array_equal(s[0], [-3.0, -17.0, -10.0]) and np.array_equal(s[1], llks[2]) and not s[2].any()
    p = tmp_path / "o.match.tsv"
    cluster.write_match_tsv(str(p), n, s, ["d0", "d1", "d2"])
    lines = p.read_text().splitlines()
    assert lines[0] == "CLUST\tSM_ID\tN.CELL\tSUM.LLK\tBEST"
    assert len(lines) == 1 + 3 * 3
    best = [ln.split("\t")[:2] for ln in lines[1:] if ln.endswith("\t1")]
    assert best == [["CLUST0", "d0"], ["CLUST1", "d1"]]          # a cluster without singlets has no BEST row
    assert lines[1] == "CLUST0\td0\t2\t-3.00000\t1"


def test_match_labels():
    rng = np.random.default_rng(3)
    truth = rng.integers(0, 5, size=400)
    perm = np.array([3, 0, 4, 1, 2])
    pred = perm[truth]
    flip = rng.random(400) < 0.1
    pred[flip] = rng.integers(0, 5, size=flip.sum())
    m = cluster.match_labels(truth, pred, 5, 5)
    assert np.array_equal(m[perm], np.arange(5))
    # more predicted labels than true ones: the extra one maps to -1; negative labels are ignored
    m = cluster.match_labels(np.array([0, 0, 1, 1, -1]), np.array([2, 2, 0, 1, 1]), 2, 3)
    assert list(m) == [1, -1, 0]
