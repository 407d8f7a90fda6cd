"""CPU: partly genotyped pools (demuxlet_amd.partial) — argument errors, the seeded start, the column helpers, CLI parsing and the
.clust.tsv / .match.tsv writers.  No GPU compute is called."""
import numpy as np
import pytest

from demuxlet_amd import cluster, partial, refine


def args(**kw):
    a = dict(n_known=3, n_unknown=2, restarts=4, known_ids=["a", "b", "c"], max_iter=10, tol=1e-7, floor=1e-3, n_cells=100, n_pairs=500)
    a.update(kw)
    return a


def test_check_args_accepts_a_normal_run():
    partial.check_args(**args())


@pytest.mark.parametrize("kw,msg", [
    (dict(n_unknown=0), "at least 1"),
    (dict(n_known=0, known_ids=[]), "demuxlet_amd.cluster"),
    (dict(restarts=0), "--restarts"),
    (dict(n_known=3, n_unknown=4, restarts=1023), "4094"),            # 3 + 4092 = 4095 columns
    (dict(known_ids=["a", "UNK1", "c"]), "collides"),
    (dict(known_ids=["a", "a", "c"]), "distinct"),
    (dict(known_ids=["a", "b"]), "sample ids"),
    (dict(max_iter=0), "--max-iter"),
    (dict(tol=-1.0), ">= 0"),
    (dict(n_pairs=0), "empty pileup"),
])
def test_check_args_errors(kw, msg):
    with pytest.raises(ValueError, match=msg):
        partial.check_args(**args(**kw))


def test_widest_engine_is_accepted():
    partial.check_args(**args(n_known=2, n_unknown=4, restarts=1023, known_ids=["a", "b"]))     # 2 + 4092 = 4094


def test_unsupported_options_raise():
    with pytest.raises(ValueError, match="not supported"):
        partial.partial_run(None, np.zeros((1, 1, 3)), ["a"], 1, "x", em_doublets=True)
    with pytest.raises(ValueError, match="not supported"):
        partial.partial_run(None, np.zeros((1, 1, 3)), ["a"], 1, "x", split_merge=True)
    with pytest.raises(ValueError, match="one GPU"):
        partial.partial_run(None, np.zeros((1, 1, 3)), ["a"], 1, "x", n_gpus=2)
    with pytest.raises(ValueError, match="not chosen automatically"):
        partial.partial_run(None, np.zeros((1, 1, 3)), ["a"], "auto", "x")


def test_initial_labels_from_llks():
    llk_known = np.array([[-5.0, -1.0, -3.0],      # explained by donor 1
                          [-2.0, -2.0, -9.0],      # a tie: the lower donor
                          [-7.0, -8.0, -9.0],      # q is better: a free column
                          [-4.0, -6.0, -4.5],      # equal to q counts as explained
                          [-9.0, -9.0, -9.0]])     # q is better
    llk_q = np.array([-2.0, -3.0, -6.0, -4.0, -1.0])
    lab = partial.initial_labels(llk_known, llk_q, seed=5, restarts=3, n_unknown=2)
    assert lab.shape == (3, 5) and lab.dtype == np.int32
    assert (lab[:, 0] == 1).all() and (lab[:, 1] == 0).all() and (lab[:, 3] == 0).all()
    rng = np.random.default_rng(5)
    for r in range(3):
        assert np.array_equal(lab[r, [2, 4]], 3 + rng.integers(0, 2, size=2))
    assert np.array_equal(lab, partial.initial_labels(llk_known, llk_q, seed=5, restarts=3, n_unknown=2))


def test_free_weights_and_random_labels():
    lab = np.array([[0, 3, 4, -1, 2], [4, 4, 1, 3, 3]], dtype=np.int32)     # Vk = 3, M = 2
    w = partial.free_weights(lab, 3, 2)
    want = np.zeros((5, 4))
    want[1, 0] = want[2, 1] = 1.0
    want[0, 3] = want[1, 3] = want[3, 2] = want[4, 2] = 1.0
    assert np.array_equal(w, want)
    mask = np.array([1, 0, 1, 1, 1], dtype=bool)
    assert not partial.free_weights(lab, 3, 2, mask)[1].any()
    rl = partial.random_labels(0, 2, 5, 3, 2)
    assert np.array_equal(rl, 3 + cluster.initial_labels(0, 2, 5, 2)) and rl.min() >= 3 and rl.max() <= 4
    with pytest.raises(ValueError, match=r"\[-1, 5\)"):
        partial.check_init_labels(np.full((1, 5), 5), 5, 3, 2)


def test_column_helpers():
    S, Vk, M, R = 4, 2, 3, 3
    gp = np.arange(S * (Vk + R * M) * 3, dtype=np.float32).reshape(S, Vk + R * M, 3)
    g = partial.final_columns(gp, Vk, M, 1)
    assert np.array_equal(g[:, :Vk], gp[:, :Vk]) and np.array_equal(g[:, Vk:], gp[:, Vk + M:Vk + 2 * M])
    q = np.full((S, 3), 0.25, dtype=np.float32)
    pr = partial.refine_prior(gp[:, :Vk], q, M)
    assert pr.shape == (S, Vk + M, 3) and pr.dtype == np.float32
    assert np.array_equal(pr[:, :Vk], gp[:, :Vk]) and (pr[:, Vk:] == 0.25).all()
    assert np.array_equal(partial.unknown_calls(np.array([-1, 0, 1, 2, 4]), 2), [-1, -1, -1, 0, 2])
    assert partial.unknown_ids(3) == ["UNK0", "UNK1", "UNK2"]


def test_parse_args():
    a = partial.parse_args(["--pileup", "x.pileup.txt", "--n-unknown", "2", "--out", "o", "--restarts", "3", "--alpha", "0", "0.25", "0.5",
                            "--rounds", "2", "--match", "--fast", "--min-snp", "5"])
    assert (a.pileup, a.n_unknown, a.out, a.restarts, a.alpha, a.rounds, a.match, a.fast, a.min_snp) == \
        ("x.pileup.txt", 2, "o", 3, [0.0, 0.25, 0.5], 2, True, True, 5)
    d = partial.parse_args(["--pileup", "p", "--n-unknown", "1", "--out", "o"])
    assert (d.restarts, d.seed, d.max_iter, d.tol, d.floor, d.rounds, d.match, d.gpu) == (16, 0, 50, 1e-7, 1e-3, 1, False, 0)
    for bad in (["--n-unknown", "0"], ["--n-unknown", "2", "--restarts", "0"], ["--n-unknown", "2", "--em-doublets"],
                ["--n-unknown", "2", "--split-merge"], ["--n-unknown", "auto"]):
        with pytest.raises(SystemExit):
            partial.parse_args(["--pileup", "p", "--out", "o"] + bad)


def test_dump_without_samples_is_an_error(tmp_path):
    p = tmp_path / "x.pileup.txt"
    p.write_text("NV\t0\nNSNP\t2\nNCELL\t1\nSNP\t0\t1\t100\tA\tG\nSNP\t1\t1\t200\tC\tT\nCELL\t0\tAAAC\t1\t1\t1\nPAIR\t1\t1\t1:30\n")
    assert refine.read_pileup_txt(str(p)).sample_ids == []
    with pytest.raises(SystemExit, match="demuxlet_amd.cluster"):
        partial.main(["--pileup", str(p), "--n-unknown", "1", "--out", str(tmp_path / "o")])


def test_clust_and_match_tsv(tmp_path):
    S, Vk, M = 3, 2, 2
    rng = np.random.default_rng(1)
    ll = rng.normal(size=(S, Vk + M, 3))
    n_cell = np.array([[1, 0, 2, 0], [0, 3, 0, 1], [1, 1, 0, 0]])
    n_ref, n_alt = n_cell * 2, n_cell
    gp = rng.dirichlet(np.ones(3), size=(S, Vk + M)).astype(np.float32)
    snps = [("1", 100 + i, "A", "G") for i in range(S)]
    partial.write_clust_tsv(str(tmp_path / "c.tsv"), snps, Vk, M, ll, n_cell, n_ref, n_alt, gp)
    rows = [ln.split("\t") for ln in (tmp_path / "c.tsv").read_text().splitlines()]
    assert rows[0] == refine.REFINED_HEADER.rstrip("\n").split("\t")
    assert [(r[1], r[4], r[5]) for r in rows[1:]] == [("100", "UNK0", "2"), ("101", "UNK1", "1")]
    assert rows[1][8] == f"{ll[0, 2, 0]:.5f}"
    n, s = cluster.match_table(rng.normal(size=(5, Vk)), np.array([0, -1, 1, 0, 1]), M)
    partial.write_match_tsv(str(tmp_path / "m.tsv"), n, s, ["d0", "d1"])
    m = [ln.split("\t") for ln in (tmp_path / "m.tsv").read_text().splitlines()]
    assert m[0] == cluster.MATCH_HEADER.rstrip("\n").split("\t")
    assert [r[:3] for r in m[1:]] == [["UNK0", "d0", "2"], ["UNK0", "d1", "2"], ["UNK1", "d0", "2"], ["UNK1", "d1", "2"]]
    assert sum(int(r[4]) for r in m[1:]) == 2
    # the clustering's rows keep their CLUST names
    cluster.write_match_tsv(str(tmp_path / "k.tsv"), n, s, ["d0", "d1"])
    assert (tmp_path / "k.tsv").read_text().splitlines()[1].startswith("CLUST0\td0\t")
