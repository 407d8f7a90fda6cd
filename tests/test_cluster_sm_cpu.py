"""CPU: the host side of the split-merge moves (demuxlet_amd/cluster.py): candidate ranking with overlap exclusion
and ties, hard labels for the splits, sub-restart seeding, split gains and posteriors, candidate weights, the .moves.tsv format,
K = 2 (no candidates), the argument checks and init_labels, and the float64 references the GPU tests use."""
import numpy as np
import pytest

import cluster_sm_ref as SM
from demuxlet_amd import cluster


def test_rank_candidates_order_and_overlap():
    K = 4                                        # pairs: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
    bf = np.array([-50.0, -10.0, -80.0, 40.0, -5.0, -90.0])
    gain = np.array([100.0, 3.0, -1.0, 30.0])
    c = cluster.rank_candidates(bf, gain, 3, 3)
    # merges (1,2), (1,3), (0,2); splits 0, 3, 1
    assert c == [(1, 2, 0), (1, 2, 3), (1, 3, 0), (0, 2, 3), (0, 2, 1)]
    assert all(m not in (k, l) for k, l, m in c)


def test_rank_candidates_ties_and_infinite_gain():
    bf = np.zeros(3)                             # K = 3: every pair ties -> pair order
    gain = np.array([5.0, 5.0, -np.inf])         # tie -> lower cluster first; -inf (too small) never split
    assert cluster.rank_candidates(bf, gain, 3, 3) == [(0, 2, 1), (1, 2, 0)]
    assert cluster.rank_candidates(bf, gain, 1, 1) == []        # merge (0,1) with split 0 overlaps
    assert cluster.rank_candidates(bf, gain, 1, 2) == []            # merge (0,1): both splits overlap


def test_k2_has_no_candidates():
    assert cluster.rank_candidates(np.array([7.0]), np.array([3.0, 4.0]), 3, 3) == []


def test_best_candidate():
    ll = np.array([-1000.00001, -1000.0, -1200.0])
    assert cluster.best_candidate(ll, 1e-7) == 0             # within tol * |LL| of the best: the better ranked wins
    assert cluster.best_candidate(ll, 0.0) == 1
    assert cluster.best_candidate(np.array([-5.0, -5.0]), 0.0) == 0


def test_split_groups():
    w = np.array([[0.2, 0.8, 0.0], [0.5, 0.5, 0.0], [0.0, 0.0, 0.0], [0.1, 0.1, 0.2], [0.0, 0.0, 1.0]])
    assert cluster.split_groups(w).tolist() == [1, 0, -1, -1, 2]      # tie -> lower; singlet mass 0.4 < 0.5 -> -1
    mask = np.array([True, True, True, True, False])
    assert cluster.split_groups(w, mask).tolist() == [1, 0, -1, -1, -1]


def test_sub_restart_seeding():
    rng = np.random.default_rng(3)
    K, Rs, B = 3, 4, 200
    group = rng.integers(-1, K, size=B).astype(np.int32)
    w = cluster.sub_restart_weights(group, K, Rs, [5, 1])
    assert w.shape == (B, K * Rs * 2)
    assert np.array_equal(w, cluster.sub_restart_weights(group, K, Rs, [5, 1]))
    assert not np.array_equal(w, cluster.sub_restart_weights(group, K, Rs, [5, 2]))
    half = np.random.default_rng([5, 1]).integers(0, 2, size=(Rs, B))
    for b in range(B):
        row = w[b]
        if group[b] < 0:
            assert not row.any()
            continue
        m = group[b]
        assert row.sum() == Rs and set(np.unique(row)) <= {0.0, 1.0}
        for s in range(Rs):
            blk = row[2 * (m * Rs + s):2 * (m * Rs + s) + 2]
            assert blk[half[s, b]] == 1.0 and blk[1 - half[s, b]] == 0.0
    # each sub-restart splits its group into two non-empty halves that differ between sub-restarts
    for m in range(K):
        mine = group == m
        cols = [w[mine, 2 * (m * Rs + s)] for s in range(Rs)]
        assert all(0 < c.sum() < mine.sum() for c in cols)
        assert len({c.tobytes() for c in cols}) == Rs


def test_split_gain_and_posteriors():
    K, Rs, B = 3, 2, 6
    group = np.array([0, 0, 1, 1, 1, 2])
    llks = -np.arange(B * K, dtype=np.float64).reshape(B, K)
    ll_sub = np.array([-1.0, -0.5, -7.0, -9.0, 0.0, 0.0])
    gain, best = cluster.split_gain(ll_sub, llks, group, Rs)
    assert best.tolist() == [1, 0, 0]
    assert gain[0] == -0.5 - (llks[0, 0] + llks[1, 0]) and gain[1] == -7.0 - llks[2:5, 1].sum() and gain[2] == -np.inf
    w_sub = np.zeros((B, K * Rs * 2))
    w_sub[0, 2 * 1:2 * 1 + 2] = [0.9, 0.1]      # cluster 0, sub-restart 1
    w_sub[1, 2 * 1:2 * 1 + 2] = [0.25, 0.75]
    w_sub[2, 2 * 2:2 * 2 + 2] = [1.0, 0.0]      # cluster 1, sub-restart 0
    s_a, s_b = cluster.split_posteriors(w_sub, group, best, Rs)
    assert np.allclose(s_a + s_b, 1.0)
    assert s_a[0, 0] == 0.9 and s_a[0, 1] == 0.25 and s_a[1, 2] == 1.0
    assert s_a[1, 3] == 0.5 and s_a[0, 5] == 0.5           # no weight / outside the group: half and half


def test_candidate_weights():
    rng = np.random.default_rng(4)
    B, K = 50, 5
    w = rng.dirichlet(np.ones(K), size=B)
    s_a = rng.random((K, B))
    s_b = 1.0 - s_a
    cands = [(1, 2, 0), (0, 3, 4)]
    out = cluster.candidate_weights(w, cands, s_a, s_b)
    assert out.shape == (B, 2 * K)
    for j, (k, l, m) in enumerate(cands):
        c = out[:, j * K:(j + 1) * K]
        assert np.array_equal(c[:, k], w[:, k] + w[:, l])
        assert np.array_equal(c[:, l], w[:, m] * s_a[m]) and np.array_equal(c[:, m], w[:, m] * s_b[m])
        rest = [x for x in range(K) if x not in (k, l, m)]
        assert np.array_equal(c[:, rest], w[:, rest])
        assert np.allclose(c.sum(axis=1), 1.0)              # no mass is lost


def test_moves_tsv(tmp_path):
    rows = [dict(move=1, cand=0, merge_k=1, merge_l=2, split=0, bf=123.4567891, gain=88.0, ll_before=-1000.5, ll_after=-990.25,
                 iterations=7, accepted=True),
            dict(move=1, cand=1, merge_k=1, merge_l=2, split=3, bf=123.4567891, gain=-2.5, ll_before=-1000.5, ll_after=-1001.0,
                 iterations=7, accepted=False)]
    p = tmp_path / "x.moves.tsv"
    cluster.write_moves_tsv(str(p), rows)
    lines = p.read_text().splitlines()
    assert lines[0] == "MOVE\tCAND\tMERGE_K\tMERGE_L\tSPLIT\tBF\tSPLIT_GAIN\tLLK_BEFORE\tLLK_AFTER\tITER\tACCEPTED"
    assert lines[1] == "1\t0\t1\t2\t0\t123.456789\t88.000000\t-1000.500000\t-990.250000\t7\t1"
    assert lines[2].split("\t")[-1] == "0" and len(lines) == 3
    cluster.write_moves_tsv(str(p), [])
    assert p.read_text() == cluster.MOVES_HEADER


def test_sm_args_and_init_labels():
    cluster.check_sm_args(16, (3, 3), 4, None)
    with pytest.raises(ValueError):
        cluster.check_sm_args(65, (3, 3), 4, None)
    with pytest.raises(ValueError):
        cluster.check_sm_args(8, (0, 3), 4, None)
    with pytest.raises(ValueError):
        cluster.check_sm_args(8, (3, 3), 4, -1)
    lab = cluster.check_init_labels(np.array([0, 1, -1, 2]), 4, 3)
    assert lab.shape == (1, 4) and lab.dtype == np.int32
    for bad in (np.array([[0, 3, 0, 0]]), np.array([[0, -2, 0, 0]]), np.zeros((1, 5), dtype=int), np.zeros((1, 4)) + 0.5):
        with pytest.raises(ValueError):
            cluster.check_init_labels(bad, 4, 3)
    w = cluster.one_hot_weights(np.array([[0, 2, -1]]), 3)
    assert w.tolist() == [[1, 0, 0], [0, 0, 1], [0, 0, 0]]


def test_cli_flags():
    a = cluster.parse_args(["--pileup", "x", "--n-clusters", "4", "--out", "o", "--split-merge", "--sm-candidates", "2", "5",
                            "--sm-split-restarts", "3", "--sm-max-moves", "1"])
    assert a.split_merge and a.sm_candidates == [2, 5] and a.sm_split_restarts == 3 and a.sm_max_moves == 1
    a = cluster.parse_args(["--pileup", "x", "--n-clusters", "4", "--out", "o"])
    assert not a.split_merge and tuple(a.sm_candidates) == cluster.SM_CANDIDATES and a.sm_max_moves is None


def test_reference_merge_score_semantics():
    """The float64 reference: a split donor's halves score positive, distinct donors negative, an empty column ~0, no shared SNP exactly 0."""
    rng = np.random.default_rng(8)
    S, K = 400, 4
    q = np.full((S, 3), 1 / 3, dtype=np.float32)
    geno = rng.integers(0, 3, size=(S, 3))                    # donors 0, 1, 2
    lgl = np.log(np.where(np.arange(3)[None, None, :] == geno[:, :, None], 0.9, 0.05))    # one read's log GL per donor, [S][3 donors][3]
    LL = np.zeros((S, K, 3))
    W = np.zeros((S, K))
    LL[:, 0], LL[:, 1], LL[:, 2] = 3 * lgl[:, 0], 3 * lgl[:, 0], 3 * lgl[:, 1]        # columns 0, 1: halves of donor 0; column 2: donor 1
    W[:, :3] = 3.0
    LL[:S // 2, 3], W[:S // 2, 3] = 3 * lgl[:S // 2, 2], 3.0                         # column 3: donor 2 on the first half of the SNPs only
    bf, ns = SM.merge_score(LL, W, q, 1e-3, 1, K)
    p = {tuple(x): i for i, x in enumerate(SM.pairs(K).tolist())}
    assert bf[0, p[(0, 1)]] > 50 and bf[0, p[(0, 2)]] < -50
    assert ns[0, p[(0, 3)]] == S // 2 and ns[0, p[(0, 1)]] == S
    W2 = W.copy()
    W2[:, 3] = 0.0
    bf2, ns2 = SM.merge_score(LL, W2, q, 1e-3, 1, K)
    assert bf2[0, p[(0, 3)]] == 0.0 and ns2[0, p[(0, 3)]] == 0


def test_reference_grouped_estep_one_group_is_plain():
    rng = np.random.default_rng(2)
    B, R, K = 40, 3, 2
    llks = rng.normal(-50, 5, size=(B, R * K))
    lp = np.log(np.full((R, K), 0.5))
    w, ll, cs = SM.estep_grouped(llks, R, K, lp, np.zeros(B, dtype=int), R)
    x = llks.reshape(B, R, K) + lp[None]
    assert np.allclose(ll, (x.max(2) + np.log(np.exp(x - x.max(2, keepdims=True)).sum(2))).sum(0))
    assert np.allclose(w.reshape(B, R, K).sum(2), 1.0)
