"""GPU (-m gpu): choosing the number of clusters (Engine.cluster_evidence / cluster_hard / cluster_merge_columns,
cluster.cluster_run(auto_k=True)).

The evidence is checked against the float64 restatement in cluster_k_ref.py (1e-9, the merge-score test's bound), for exact zeros on an
empty column, for the same bits whatever the restart's position and whatever ran before, at the chunk edges, and against the merge score
(the evidence of a merged column minus its two parts is the pair's Bayes factor).  The hard labels, counts and one-hot matrix are compared
exactly with the restatement computed from the device's own weights, doublet mass and LLD, with inactive columns, a mask and constructed
ties; the column merge bit for bit against numpy.  The existing E-steps are pinned to give exact zeros for a column with log pi = -inf.
Then the merge path end to end: it recovers 4 donors from K_max = 8 with and without doublets, keeps K = K_max = 4, writes .kpath.tsv, and
the CLI."""
import re

import numpy as np
import pytest

import cluster_k_ref as KR
import cluster_sm_ref as SM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import build, capi, cluster, engine, refine, synth
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return dict(torch=torch, capi=capi, cluster=cluster, engine=engine, refine=refine, synth=synth)


def host_pileup(m, sp):
    return m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads,
                                  sp.rd_totl, sp.rd_pass, sp.rd_uniq)


def staged(m, sp, C):
    e = m["engine"].Engine(C, (0.0, 0.5), 0.5)
    e.set_genotypes(np.full((sp.n_snps, C, 3), 1 / 3, dtype=np.float32))
    e.set_pileup(host_pileup(m, sp))
    e.cluster_stage()
    return e


def synth_case(m, K, seed, B=4000, S=10000, delta=0.1, rbar=1.25, doublet_rate=0.1, dense=False):
    rng = np.random.default_rng(seed)
    raw = m["synth"].make_raw_genotypes(rng, S, K)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, delta, rbar, dense_layout=dense, doublet_rate=doublet_rate)
    return raw, sp, host_pileup(m, sp), [m["synth"].barcode_name(c) for c in range(B)]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def close(a, ref, rel=1e-9):
    return bool((np.abs(a - ref) <= rel * np.maximum(np.abs(ref), 1.0)).all())


def donor_weights(truth, donors):
    """[B][len(donors)] one-hot of each barcode's first true donor among `donors` (a donor may repeat: identical columns)."""
    return np.stack([(truth[:, 0] == d).astype(np.float64) for d in donors], axis=1)


# ---- evidence ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [False, True])
def test_evidence_parity(m, dense):
    rng = np.random.default_rng(171 + dense)
    S, B = (600, 150) if dense else (3000, 300)
    K = 5
    _, sp, _, _ = synth_case(m, 4, 171 + dense, B=B, S=S, delta=1.0 if dense else 0.1, rbar=1.5, dense=dense)
    q = m["cluster"].hwe_prior(rng.integers(0, 50, S), rng.integers(0, 50, S))
    w1 = rng.random((B, K))
    w1[:, 3] = 0.0                                         # an empty column: W = 0 at every SNP
    w1[: B // 2, 4] = 0.0                                  # a column that is zero for half the barcodes
    a = staged(m, sp, K)
    b = staged(m, sp, 3 * K)
    try:
        LL, W, _ = a.cluster_mstep(w1, q, 1e-3)
        ev, nc = a.cluster_evidence(1, K, q, 1e-3)
        rev, rnc = KR.evidence(LL, W, q, 1e-3, 1, K)
        assert np.array_equal(nc, rnc)
        assert close(ev, rev), np.abs(ev - rev).max()
        assert ev[0, 3] == 0.0 and nc[0, 3] == 0 and not np.signbit(ev[0, 3])
        assert (nc[0, [0, 1, 2]] > 0).all() and 0 < nc[0, 4] <= nc[0, 0]
        inf = a.cluster_k_info()
        assert inf["n_restarts"] == 1 and inf["n_clusters"] == K and inf["n_chunks"] == (S + 255) // 256 and inf["evidence_ms"] > 0
        # against the merge score: the merged column's evidence minus its two parts is the pair's Bayes factor
        bf, ns = a.cluster_merge_score(1, K, q, 1e-3)
        pidx = {tuple(x): i for i, x in enumerate(SM.pairs(K).tolist())}
        for k, l in ((0, 1), (1, 2), (0, 4), (2, 3)):
            wm = w1.copy()
            wm[:, k] = w1[:, k] + w1[:, l]
            wm[:, l] = 0.0
            a.cluster_mstep(wm, q, 1e-3, fetch=False)
            evm, _ = a.cluster_evidence(1, K, q, 1e-3)
            d = evm[0, k] - ev[0, k] - ev[0, l]
            assert abs(d - bf[0, pidx[(k, l)]]) <= 1e-9 * max(abs(evm[0, k]), 1.0), (k, l, d, bf[0, pidx[(k, l)]])
            assert evm[0, l] == 0.0
        # the same K columns as restart 2 of R = 3, and after unrelated engine calls
        w3 = np.concatenate([rng.random((B, K)), rng.random((B, K)), w1], axis=1)
        LL3, W3, _ = b.cluster_mstep(w3, q, 1e-3)
        ev3, nc3 = b.cluster_evidence(3, K, q, 1e-3)
        assert np.array_equal(bits(ev3[2]), bits(ev[0])) and np.array_equal(nc3[2], nc[0])
        rev3, rnc3 = KR.evidence(LL3, W3, q, 1e-3, 3, K)
        assert close(ev3, rev3) and np.array_equal(nc3, rnc3)
        a.run_singlet()
        a.cluster_estep(1, K, np.full((1, K), -np.log(K)))
        a.cluster_hard(1, K, np.ones((1, K)))
        a.cluster_mstep(w1, q, 1e-3, fetch=False)
        a.cluster_merge_score(1, K, q, 1e-3)
        again, nagain = a.cluster_evidence(1, K, q, 1e-3)
        assert np.array_equal(bits(again), bits(ev)) and np.array_equal(nagain, nc)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("S", [256, 257, 1])
def test_evidence_chunk_edges(m, S):
    rng = np.random.default_rng(900 + S)
    B, R, K = 60, 2, 3
    _, sp, _, _ = synth_case(m, 3, 900 + S, B=B, S=S, delta=0.6, rbar=1.5, doublet_rate=0.0)
    q = m["cluster"].hwe_prior(rng.integers(0, 20, S), rng.integers(0, 20, S))
    e = staged(m, sp, R * K)
    try:
        w = rng.random((B, R * K))
        w[:, 4] = 0.0
        LL, W, _ = e.cluster_mstep(w, q, 1e-3)
        ev, nc = e.cluster_evidence(R, K, q, 1e-3)
        rev, rnc = KR.evidence(LL, W, q, 1e-3, R, K)
        assert np.array_equal(nc, rnc) and close(ev, rev)
        assert ev[1, 1] == 0.0 and nc[1, 1] == 0
        assert e.cluster_k_info()["n_chunks"] == (S + 255) // 256
    finally:
        e.close()


# ---- hard labels ---------------------------------------------------------------------------------------------------------------------------
def hard_setup(m, sp, cols, log_pi, R, K, q, mask, log_delta):
    """An engine whose last E-step (the doublet one when log_delta is given) ran on the genotypes of an M-step of `cols`."""
    e = staged(m, sp, R * K)
    e.cluster_mstep(cols, q, 1e-3, fetch=False)
    e.set_genotypes_device(e.cluster_device_ptr(), sp.n_snps)
    e.run_singlet()
    if log_delta is None:
        e.cluster_estep(R, K, log_pi, 1.0, mask)
    else:
        e.cluster_doublet(R, K)
        e.cluster_estep_doublet(R, K, log_pi, log_delta, 1.0, mask)
    return e


def check_hard(e, R, K, active, mask, doublets):
    """cluster_hard against the restatement computed from the device's own weights, doublet mass and LLD; returns the device's results."""
    w0 = e.cluster_weights()
    label, n_sing, n_dbl, score = e.cluster_hard(R, K, active, mask, doublets=doublets)
    assert np.array_equal(bits(e.cluster_weights()), bits(w0))          # the E-step's weights are only read
    if doublets:
        lab_d, dsc, hot, dm = e.get_cluster_hard(R, K, dbl_mass=True)
        lld, _ = e.get_cluster_doublet()
    else:
        lab_d, dsc, hot = e.get_cluster_hard(R, K)
        dm = lld = None
    assert np.array_equal(lab_d, label)
    rl, rn, rd, rs, rhot = KR.hard(w0, active, R, K, mask, dm, lld)
    assert np.array_equal(label, rl) and np.array_equal(n_sing, rn) and np.array_equal(n_dbl, rd)
    assert np.array_equal(bits(hot), bits(rhot))
    assert close(score, rs), (score, rs)
    if doublets:
        on = label <= -2
        assert np.array_equal(dsc[on], np.take_along_axis(lld, np.maximum(-2 - label, 0)[:, :, None], axis=2)[:, :, 0][on]) and not dsc[~on].any()
    else:
        assert not dsc.any() and not score.any() and not n_dbl.any()
    return w0, label, n_sing, n_dbl, score, dm, lld


def test_hard_labels(m):
    R, K, B, S = 2, 4, 300, 3000
    _, sp, _, _ = synth_case(m, 4, 33, B=B, S=S, delta=0.1, rbar=1.5, doublet_rate=0.3)
    q = m["cluster"].hwe_prior(np.zeros(S), np.zeros(S))
    rng = np.random.default_rng(33)
    mask = rng.random(B) < 0.85
    # restart 0: columns 0 and 1 are the same donor (exact ties in w, and in LLD between the pairs (0, 2) and (1, 2)), column 3 is inactive;
    # restart 1: the four donors, column 1 inactive
    r0, r1 = donor_weights(sp.truth, [0, 0, 1, 2]), donor_weights(sp.truth, [0, 1, 2, 3])
    active = np.array([[1, 1, 1, 0], [1, 0, 1, 1]], dtype=np.uint8)
    with np.errstate(divide="ignore"):
        lp0, lp1 = np.log([0.3, 0.3, 0.4, 0.0]), np.log([0.3, 0.0, 0.3, 0.4])
    log_delta = np.log([0.2, 0.2])
    a = hard_setup(m, sp, np.concatenate([r0, r1], axis=1), np.stack([lp0, lp1]), R, K, q, mask, log_delta)
    b = hard_setup(m, sp, np.concatenate([r1, r0], axis=1), np.stack([lp1, lp0]), R, K, q, mask, log_delta)    # the restarts swapped
    c = hard_setup(m, sp, np.concatenate([r0, r1], axis=1), np.stack([lp0, lp1]), R, K, q, mask, None)         # the plain E-step
    try:
        w, label, n_sing, n_dbl, score, dm, lld = check_hard(a, R, K, active, mask, True)
        assert (label[~mask] == -1).all() and (label[mask] != -1).all()
        assert not w[:, [3, 5]].any() and n_sing[0, 3] == 0 and n_sing[1, 1] == 0
        assert (n_dbl > 10).all() and (n_sing.sum(axis=1) > 100).all() and (n_sing.sum(axis=1) + n_dbl == mask.sum()).all()
        # the constructed ties happened, and went to the lower index
        tie_w = mask & (w[:, 0] == w[:, 1]) & (w[:, 0] > w[:, 2]) & (dm[:, 0] < 0.5)
        assert tie_w.sum() > 20 and (label[tie_w, 0] == 0).all()
        tie_d = mask & (dm[:, 0] >= 0.5) & (lld[:, 0, 1] == lld[:, 0, 3]) & (lld[:, 0, 1] > lld[:, 0, 0])
        assert tie_d.sum() > 2 and (label[tie_d, 0] == -2 - 1).all()
        assert not np.isin(label[:, 0], [-2 - 2, -2 - 4, -2 - 5, 3]).any()       # no pair with, and no label of, the inactive column 3
        assert not np.isin(label[:, 1], [-2 - 0, -2 - 3, -2 - 4, 1]).any()
        # the same bits on repeat, and with the restarts in the other order
        again = a.cluster_hard(R, K, active, mask, doublets=True)
        assert np.array_equal(bits(again[3]), bits(score)) and np.array_equal(again[0], label)
        _, label_b, n_sing_b, n_dbl_b, score_b, _, _ = check_hard(b, R, K, active[::-1], mask, True)
        assert np.array_equal(label_b, label[:, ::-1]) and np.array_equal(n_sing_b, n_sing[::-1]) and np.array_equal(n_dbl_b, n_dbl[::-1])
        assert np.array_equal(bits(score_b), bits(score[::-1]))
        inf = a.cluster_k_info()
        assert inf["hard_ms"] > 0 and inf["n_cells"] == B
        # without doublet labels: every barcode of the mask is a singlet of an active column; the one-hot matrix feeds the M-step
        _, label_p, n_sing_p, _, _, _, _ = check_hard(a, R, K, active, mask, False)
        assert (n_sing_p.sum(axis=1) == mask.sum()).all() and (label_p[mask] >= 0).all()
        _, _, hot = a.get_cluster_hard(R, K)
        dev = a.cluster_mstep(a.cluster_hard_device_ptr(), q, 1e-3)
        host = a.cluster_mstep(hot, q, 1e-3)
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(dev, host))
        check_hard(c, R, K, active, mask, False)
        check_hard(c, R, K, active, None, False)
    finally:
        a.close()
        b.close()
        c.close()


@pytest.mark.parametrize("B", [256, 257, 1])
def test_hard_labels_chunk_edges(m, B):
    R, K, S = 2, 3, 400
    _, sp, _, _ = synth_case(m, 3, 700 + B, B=B, S=S, delta=0.3, rbar=1.5, doublet_rate=0.5)
    q = m["cluster"].hwe_prior(np.zeros(S), np.zeros(S))
    cols = np.concatenate([donor_weights(sp.truth, [0, 1, 2]), donor_weights(sp.truth, [2, 0, 1])], axis=1)
    e = hard_setup(m, sp, cols, np.full((R, K), -np.log(K)), R, K, q, None, np.log([0.45, 0.45]))
    try:
        _, label, n_sing, n_dbl, score, _, _ = check_hard(e, R, K, np.ones((R, K)), None, True)
        assert (n_sing.sum(axis=1) + n_dbl == B).all()
        if B > 1:
            assert (n_dbl > 5).all() and score.all()
        check_hard(e, R, K, np.array([[1, 1, 0], [0, 1, 1]]), None, True)
        check_hard(e, R, K, np.array([[1, 0, 0], [0, 1, 1]]), None, False)
    finally:
        e.close()


# ---- column merge --------------------------------------------------------------------------------------------------------------------------
def test_merge_columns(m):
    R, K, B, S = 3, 4, 300, 2000
    _, sp, _, _ = synth_case(m, 4, 44, B=B, S=S, delta=0.1, rbar=1.5)
    q = m["cluster"].hwe_prior(np.zeros(S), np.zeros(S))
    rng = np.random.default_rng(44)
    e = hard_setup(m, sp, rng.random((B, R * K)), np.log(rng.dirichlet(np.ones(K), size=R)), R, K, q, None, None)
    try:
        w0 = e.cluster_weights()
        frm, into = [2, -1, 0], [0, 0, 3]
        e.cluster_merge_columns(R, K, frm, into)
        w1 = e.cluster_weights()
        assert np.array_equal(bits(w1), bits(KR.merge_columns(w0, R, K, frm, into)))
        assert np.array_equal(bits(w1[:, K:2 * K]), bits(w0[:, K:2 * K]))             # from = -1: untouched
        assert not w1[:, 2].any() and not w1[:, 2 * K].any() and np.array_equal(w1[:, 0], w0[:, 0] + w0[:, 2])
        assert e.cluster_k_info()["merge_columns_ms"] > 0
        last = e.cluster_mstep(None, q, 1e-3)              # DMX_CLUSTER_LAST_ESTEP: no host round trip
        host = e.cluster_mstep(w1, q, 1e-3)
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(last, host))
    finally:
        e.close()


# ---- inactive columns through the existing E-steps -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("doublets", [False, True])
def test_inactive_columns_get_exact_zeros(m, doublets):
    R, K, B, S = 2, 4, 300, 2000
    _, sp, _, _ = synth_case(m, 4, 55, B=B, S=S, delta=0.1, rbar=1.5, doublet_rate=0.2)
    q = m["cluster"].hwe_prior(np.zeros(S), np.zeros(S))
    rng = np.random.default_rng(55)
    cols = np.concatenate([donor_weights(sp.truth, [0, 1, 2, 3]), donor_weights(sp.truth, [3, 2, 1, 0])], axis=1)
    off = 2                                                # column 2 of every restart is inactive
    keep = np.array([c for c in range(R * K) if c % K != off])
    pi = rng.dirichlet(np.ones(K - 1), size=R)
    with np.errstate(divide="ignore"):
        lp_full = np.log(np.insert(pi, off, 0.0, axis=1))
    mask = rng.random(B) < 0.9
    ld = np.log([0.15, 0.3]) if doublets else None
    a = hard_setup(m, sp, cols, lp_full, R, K, q, mask, ld)
    b = hard_setup(m, sp, cols[:, keep], np.log(pi), R, K - 1, q, mask, ld)
    try:
        if doublets:
            ll_a, cs_a, dm_a = a.cluster_estep_doublet(R, K, lp_full, ld, 1.0, mask)
            ll_b, cs_b, dm_b = b.cluster_estep_doublet(R, K - 1, np.log(pi), ld, 1.0, mask)
            assert np.array_equal(bits(dm_a), bits(dm_b))
        else:
            ll_a, cs_a = a.cluster_estep(R, K, lp_full, 1.0, mask)
            ll_b, cs_b = b.cluster_estep(R, K - 1, np.log(pi), 1.0, mask)
        w_a, w_b = a.cluster_weights(), b.cluster_weights()
        assert np.isfinite(ll_a).all() and np.isfinite(w_a).all()
        assert not w_a[:, off::K].any() and not np.signbit(w_a[:, off::K]).any() and not cs_a[off::K].any()
        assert np.array_equal(bits(ll_a), bits(ll_b))
        assert np.array_equal(bits(w_a[:, keep]), bits(w_b)) and np.array_equal(bits(cs_a[keep]), bits(cs_b))
    finally:
        a.close()
        b.close()


# ---- error codes ---------------------------------------------------------------------------------------------------------------------------
def test_error_codes(m):
    capi = m["capi"]
    B, S = 100, 500
    _, sp, _, _ = synth_case(m, 3, 5, B=B, S=S)
    q = m["cluster"].hwe_prior(np.zeros(S), np.zeros(S))
    e = staged(m, sp, 6)

    def fails(code, fn, *a, **kw):
        with pytest.raises(capi.DmxError) as ex:
            fn(*a, **kw)
        assert ex.value.code == code, ex.value

    try:
        ones = np.ones((2, 3))
        fails(capi.DMX_ERR_STATE, e.cluster_evidence, 2, 3, q)                   # before an M-step
        fails(capi.DMX_ERR_STATE, e.cluster_hard, 2, 3, ones)                    # before an E-step
        fails(capi.DMX_ERR_STATE, e.cluster_merge_columns, 2, 3, [0, 0], [1, 1])
        fails(capi.DMX_ERR_STATE, e.cluster_hard_device_ptr)
        e.cluster_mstep(np.ones((B, 6)), q, fetch=False)
        fails(capi.DMX_ERR_ARG, e.cluster_evidence, 1, 3, q)                     # 3 != the M-step's 6 columns
        fails(capi.DMX_ERR_ARG, e.cluster_evidence, 6, 1, q[:0])                 # a missing prior
        fails(capi.DMX_ERR_ARG, e.cluster_evidence, 0, 0, q)
        e.cluster_evidence(6, 1, q)                                              # K = 1 is allowed
        e.set_genotypes_device(e.cluster_device_ptr(), S)
        e.run_singlet()
        e.cluster_estep(2, 3, np.full((2, 3), -np.log(3)))
        fails(capi.DMX_ERR_ARG, e.cluster_hard, 3, 3, np.ones((3, 3)))           # 9 != the weights' 6 columns
        fails(capi.DMX_ERR_ARG, e.cluster_hard, 2, 3, np.array([[1, 1, 1], [0, 0, 0]]))    # a restart with no active column
        fails(capi.DMX_ERR_STATE, e.cluster_hard, 2, 3, ones, doublets=True)     # no doublet likelihoods
        e.cluster_doublet(2, 3)
        fails(capi.DMX_ERR_STATE, e.cluster_hard, 2, 3, ones, doublets=True)     # LLD, but the last E-step left no doublet mass
        e.cluster_estep_doublet(2, 3, np.full((2, 3), -np.log(3)), np.log([0.1, 0.1]))
        fails(capi.DMX_ERR_ARG, e.cluster_hard, 2, 3, np.array([[1, 1, 1], [0, 1, 0]]), doublets=True)   # fewer than two active columns
        e.cluster_hard(2, 3, np.array([[1, 1, 1], [0, 1, 0]]))
        fails(capi.DMX_ERR_STATE, e.get_cluster_hard, 2, 3, dbl_mass=True)       # those labels read no doublet mass
        e.cluster_hard(2, 3, ones, doublets=True)
        e.cluster_estep(2, 3, np.full((2, 3), -np.log(3)))
        fails(capi.DMX_ERR_STATE, e.cluster_hard, 2, 3, ones, doublets=True)     # a plain E-step since: the doublet mass is stale
        fails(capi.DMX_ERR_ARG, e.cluster_merge_columns, 3, 3, [0, 0, 0], [1, 1, 1])
        fails(capi.DMX_ERR_ARG, e.cluster_merge_columns, 2, 3, [1, -1], [1, 0])  # from == into
        fails(capi.DMX_ERR_ARG, e.cluster_merge_columns, 2, 3, [3, -1], [0, 0])  # outside [0, K)
        fails(capi.DMX_ERR_ARG, e.cluster_merge_columns, 2, 3, [0, 1], [1, -1])
        fails(capi.DMX_ERR_ARG, e.cluster_merge_columns, 2, 3, [-2, 1], [1, 0])
        e.cluster_merge_columns(2, 3, [-1, -1], [7, -5])                         # into is not read where from = -1
    finally:
        e.close()


def test_evidence_k_range(m):
    B, S = 50, 300
    _, sp, _, _ = synth_case(m, 3, 6, B=B, S=S)
    q = m["cluster"].hwe_prior(np.zeros(S), np.zeros(S))
    e = staged(m, sp, 65)
    try:
        e.cluster_mstep(np.ones((B, 65)), q, fetch=False)
        with pytest.raises(m["capi"].DmxError) as ex:
            e.cluster_evidence(1, 65, q)                   # K outside [1, 64]
        assert ex.value.code == m["capi"].DMX_ERR_ARG
        ev, nc = e.cluster_evidence(65, 1, q)
        assert ev.shape == (65, 1) and (nc > 0).all()
    finally:
        e.close()


# ---- the merge path end to end -------------------------------------------------------------------------------------------------------------
def read_best(path):
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        col = {n: i for i, n in enumerate(head)}
        return {t[col["BARCODE"]]: t[col["BEST"]] for t in (ln.rstrip("\n").split("\t") for ln in f)}


def accuracy(m, truth, barcodes, prefix, n_donors, K):
    """(share of true singlets called SNG- of their donor's cluster after greedy label matching, share of true doublets called DBL-)."""
    best = read_best(prefix + ".best")
    calls = [best.get(b, "") for b in barcodes]
    sng = np.array([int(c[len("SNG-CLUST"):]) if c.startswith("SNG-") else -1 for c in calls])
    is_dbl = np.array([c.startswith("DBL-") for c in calls])
    singlet = truth[:, 1] < 0
    lab = m["cluster"].match_labels(np.where(singlet, truth[:, 0], -1), sng, n_donors, K)
    mapped = np.where(sng >= 0, lab[np.maximum(sng, 0)], -1)
    return float((mapped == truth[:, 0])[singlet].mean()), float(is_dbl[~singlet].mean()) if (~singlet).any() else 1.0


def recovery_case(m, seed, rate):
    return synth_case(m, 4, seed, B=800, S=4000, delta=0.15, rbar=1.25, doublet_rate=rate)


def check_kpath(m, prefix, res, k_max, k_min, R):
    """.kpath.tsv: (k_max - k_min + 1) * R rows and exactly one CHOSEN, whose SCORE exceeds that of every row at another K and is not below
    any row's (two restarts that reach the same clustering score the same; the tie goes to the lower restart).  Returns the margins to
    the runner-up row and to the best row at another K."""
    lines = open(prefix + ".kpath.tsv").read().splitlines()
    assert lines[0] + "\n" == m["cluster"].KPATH_HEADER
    head = lines[0].split("\t")
    rows = [dict(zip(head, ln.split("\t"))) for ln in lines[1:]]
    assert len(rows) == (k_max - k_min + 1) * R == len(res["kpath"])
    assert [(int(r["STEP"]), int(r["RESTART"]), int(r["K"])) for r in rows] == [(t, r, k_max - t) for t in range(k_max - k_min + 1) for r in range(R)]
    chosen = [r for r in rows if r["CHOSEN"] == "1"]
    assert len(chosen) == 1 and int(chosen[0]["K"]) == res["n_clusters"] and int(chosen[0]["RESTART"]) == res["restart"]
    others = [float(r["SCORE"]) for r in rows if r["CHOSEN"] != "1"]
    assert all(float(chosen[0]["SCORE"]) >= s for s in others)
    assert all(float(chosen[0]["SCORE"]) > float(r["SCORE"]) for r in rows if int(r["K"]) != res["n_clusters"])
    i = next(i for i, r in enumerate(res["kpath"]) if r["chosen"])
    assert m["cluster"].path_winner(res["kpath"]) == i and rows[i]["CHOSEN"] == "1"
    for r in rows:
        assert len(r["SIZES"].split(",")) == int(r["K"]) and sum(int(x) for x in r["SIZES"].split(",")) == int(r["N.SNG"])
        assert abs(float(r["SCORE"]) - (float(r["EVIDENCE"]) + float(r["DBL.SCORE"]) + float(r["LABEL.TERM"]))) < 1e-5
        assert (r["BF"] == "NA") == (int(r["K"]) == k_min)
    other_k = [float(r["SCORE"]) for r in rows if int(r["K"]) != res["n_clusters"]]
    return float(chosen[0]["SCORE"]) - max(others) if others else float("inf"), float(chosen[0]["SCORE"]) - max(other_k) if other_k else float("inf")


@pytest.mark.parametrize("seed", [1, 2])
def test_recovers_four_donors_without_doublets(m, tmp_path, seed):
    raw, sp, pl, barcodes = recovery_case(m, seed, 0.0)
    pre = str(tmp_path / "a")
    res = m["cluster"].cluster_run(pl, 8, pre, restarts=2, seed=seed, barcodes=barcodes, auto_k=True)
    margin, margin_k = check_kpath(m, pre, res, 8, 2, 2)
    best_by_k = {k: max(r["score"] for r in res["kpath"] if r["k"] == k) for k in range(2, 9)}
    print(f"auto-k no doublets seed {seed}: K* = {res['n_clusters']}, margin to the runner-up row {margin:.1f}, to the best other K {margin_k:.1f}; "
          + ", ".join(f"K={k}: {s:.1f}" for k, s in sorted(best_by_k.items())))
    assert res["n_clusters"] == 4 and res["gp"].shape == (4000, 4, 3)
    sng, _ = accuracy(m, sp.truth, barcodes, pre, 4, 4)
    print(f"  singlets right {sng:.4f}")
    assert sng == 1.0
    names = {c for c in read_best(pre + ".best").values()}
    assert {c for c in names if c.startswith("SNG-")} == {f"SNG-CLUST{k}" for k in range(4)}
    em = open(pre + ".em.tsv").read().splitlines()
    assert int(em[-1].split("\t")[0]) > res["iterations"]                    # the path went on below K*: its iterations are appended
    assert any("0" in ln.split("\t")[3].split(",") for ln in em[1:])           # a merged column's pi is printed as 0


@pytest.mark.parametrize("seed", [1, 2])
def test_recovers_four_donors_with_doublets(m, tmp_path, seed):
    raw, sp, pl, barcodes = recovery_case(m, seed, 0.1)
    pre = str(tmp_path / "d")
    res = m["cluster"].cluster_run(pl, 8, pre, restarts=2, seed=seed, barcodes=barcodes, auto_k=True, em_doublets=True)
    margin, margin_k = check_kpath(m, pre, res, 8, 2, 2)
    best_by_k = {k: max(r["score"] for r in res["kpath"] if r["k"] == k) for k in range(2, 9)}
    sng, dbl = accuracy(m, sp.truth, barcodes, pre, 4, res["n_clusters"])
    print(f"auto-k 10 % doublets, em_doublets, seed {seed}: K* = {res['n_clusters']}, margin to the runner-up row {margin:.1f}, to the best other K "
          f"{margin_k:.1f}; singlets right {sng:.4f}, true doublets called DBL- {dbl:.4f}; "
          + ", ".join(f"K={k}: {s:.1f}" for k, s in sorted(best_by_k.items())))
    assert res["n_clusters"] == 4
    assert sng == 1.0


def test_kmax_equal_to_k_true(m, tmp_path):
    raw, sp, pl, barcodes = recovery_case(m, 1, 0.0)
    pre = str(tmp_path / "c")
    res = m["cluster"].cluster_run(pl, 4, pre, restarts=2, seed=1, barcodes=barcodes, auto_k=True)
    margin, _ = check_kpath(m, pre, res, 4, 2, 2)
    print(f"auto-k K_max = 4 = K_true: K* = {res['n_clusters']}, margin {margin:.1f}")
    assert res["n_clusters"] == 4
    res3 = m["cluster"].cluster_run(pl, 4, str(tmp_path / "c3"), restarts=2, seed=1, barcodes=barcodes, auto_k=True, k_min=4)
    check_kpath(m, str(tmp_path / "c3"), res3, 4, 4, 2)
    assert res3["n_clusters"] == 4
    # without the flag nothing changes: no .kpath.tsv, no new keys
    plain = m["cluster"].cluster_run(pl, 4, str(tmp_path / "p"), restarts=2, seed=1, barcodes=barcodes)
    assert not (tmp_path / "p.kpath.tsv").exists() and "kpath" not in plain and "n_clusters" not in plain


def test_cli_auto_k(m, tmp_path):
    raw, sp, pl, barcodes = recovery_case(m, 1, 0.0)
    g = np.stack([m["engine"].geno_from_gt(raw.alleles[s], 0.01) for s in range(sp.n_snps)])
    d = m["refine"].PileupDump([f"s{v}" for v in range(4)], [(1, 100 + s, "A", "G") for s in range(sp.n_snps)], g, barcodes, pl)
    p = tmp_path / "x.pileup.txt"
    m["refine"].write_pileup_txt(str(p), d)
    assert m["cluster"].main(["--pileup", str(p), "--n-clusters", "8", "--out", str(tmp_path / "c"), "--restarts", "2", "--seed", "1", "--auto-k"]) == 0
    for ext in (".best", ".single", ".sing2", ".r1.best", ".em.tsv", ".clust.tsv", ".kpath.tsv"):
        assert (tmp_path / ("c" + ext)).stat().st_size > 0, ext
    assert (tmp_path / "c.kpath.tsv").read_text().startswith(m["cluster"].KPATH_HEADER)
    names = set()
    for c in read_best(str(tmp_path / "c.best")).values():
        names.update(re.findall(r"CLUST\d+", c))
    assert names == {f"CLUST{k}" for k in range(4)}
