"""GPU (-m gpu): split-merge moves for the genotype-free EM (Engine.cluster_merge_score / cluster_estep_grouped,
cluster.cluster_run(split_merge=True)).

The merge scores are checked against the float64 restatement in cluster_sm_ref.py (1e-9), for exact zeros without shared SNPs, and for
the same bits whatever the restart's position and whatever ran before; the grouped E-step against numpy (1e-12) and, with one group,
bit for bit against cluster_estep.  Then the moves end to end: a planted local optimum (two donors in one cluster, one donor split over
two) that plain EM keeps and the moves repair, with and without doublet components; single restarts at K = 8; the cfg6 shape at K = 16;
no change where EM is already right; the CLI."""
import time

import numpy as np
import pytest

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


def read_best(path):
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        col = {n: i for i, n in enumerate(head)}
        return {t[col["BARCODE"]]: t[col["BEST"]] for t in (ln.rstrip("\n").split("\t") for ln in f)}


def accuracy(m, truth, barcodes, prefix, K):
    """(share of true singlets called SNG- of the right cluster, share of true doublets called DBL-, per-donor share of its singlets in
    its matched cluster), after greedy label matching."""
    best = read_best(prefix + ".best")
    calls = [best.get(b, "") for b in barcodes]
    sng = np.array([int(c[len("SNG-CLUST"):]) if c.startswith("SNG-") else -1 for c in calls])
    is_dbl = np.array([c.startswith("DBL-") for c in calls])
    singlet = truth[:, 1] < 0
    truth_s = np.where(singlet, truth[:, 0], -1)
    lab = m["cluster"].match_labels(truth_s, sng, K, K)
    mapped = np.where(sng >= 0, lab[np.maximum(sng, 0)], -1)
    ok = mapped == truth[:, 0]
    per = np.array([ok[singlet & (truth[:, 0] == t)].mean() for t in range(K)])
    return float(ok[singlet].mean()), float(is_dbl[~singlet].mean()) if (~singlet).any() else 1.0, per


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


@pytest.mark.parametrize("dense", [False, True])
def test_merge_score_parity(m, dense):
    rng = np.random.default_rng(71 + dense)
    S, B = (600, 150) if dense else (3000, 300)
    K = 5
    _, sp, _, _ = synth_case(m, 4, 71 + dense, B=B, S=S, delta=1.0 if dense else 0.1, rbar=1.5, dense=dense)
    q = m["cluster"].hwe_prior(rng.integers(0, 50, S), rng.integers(0, 50, S))
    w1 = rng.random((B, K))
    w1[:, 3] = 0.0                                         # an empty column: W = 0 at every SNP
    w1[: B // 2, 4] = 0.0                                  # a column covering only some SNPs
    a = staged(m, sp, K)
    b = staged(m, sp, 3 * K)
    try:
        LL, W, _ = a.cluster_mstep(w1, q, 1e-3)
        bf, ns = a.cluster_merge_score(1, K, q, 1e-3)
        rbf, rns = SM.merge_score(LL, W, q, 1e-3, 1, K)
        assert np.array_equal(ns, rns)
        assert (np.abs(bf - rbf) <= 1e-9 * np.maximum(np.abs(rbf), 1.0)).all(), np.abs(bf - rbf).max()
        p = {tuple(x): i for i, x in enumerate(SM.pairs(K).tolist())}
        for k in range(K):
            if k != 3:
                pk = p[tuple(sorted((k, 3)))]
                assert bf[0, pk] == 0.0 and ns[0, pk] == 0
        inf = a.cluster_sm_info()
        assert inf["n_pairs"] == K * (K - 1) // 2 and inf["n_chunks"] == (S + 255) // 256 and inf["merge_ms"] > 0
        # the same K columns as restart 2 of R = 3, and after unrelated engine calls
        w3 = np.concatenate([rng.random((B, K)), rng.random((B, K)), w1], axis=1)
        LL3, W3, _ = b.cluster_mstep(w3, q, 1e-3)
        bf3, ns3 = b.cluster_merge_score(3, K, q, 1e-3)
        assert np.array_equal(bits(bf3[2]), bits(bf[0])) and np.array_equal(ns3[2], ns[0])
        rbf3, _ = SM.merge_score(LL3, W3, q, 1e-3, 3, K)
        assert (np.abs(bf3 - rbf3) <= 1e-9 * np.maximum(np.abs(rbf3), 1.0)).all()
        a.run_singlet()
        a.cluster_estep(1, K, np.full((1, K), -np.log(K)))
        a.cluster_mstep(w1, q, 1e-3, fetch=False)
        again, _ = a.cluster_merge_score(1, K, q, 1e-3)
        assert np.array_equal(bits(again), bits(bf))
    finally:
        a.close()
        b.close()


def test_merge_score_errors(m):
    _, sp, _, _ = synth_case(m, 3, 5, B=100, S=500)
    q = m["cluster"].hwe_prior(np.zeros(500), np.zeros(500))
    e = staged(m, sp, 6)
    try:
        with pytest.raises(m["capi"].DmxError) as ex:
            e.cluster_merge_score(2, 3, q)
        assert ex.value.code == m["capi"].DMX_ERR_STATE
        e.cluster_mstep(np.ones((100, 6)), q, fetch=False)
        with pytest.raises(m["capi"].DmxError) as ex:
            e.cluster_merge_score(1, 3, q)                 # 3 != the M-step's 6 columns
        assert ex.value.code == m["capi"].DMX_ERR_ARG
        e.run_singlet()
        with pytest.raises(m["capi"].DmxError) as ex:
            e.cluster_estep_grouped(3, 2, np.zeros((3, 2)), np.full(100, 3, dtype=np.int32), 1)    # groups are -1 .. 2
        assert ex.value.code == m["capi"].DMX_ERR_ARG
    finally:
        e.close()


def test_estep_grouped_parity(m):
    rng = np.random.default_rng(19)
    S, B, R, K, Rs = 1500, 500, 6, 2, 2
    _, sp, _, _ = synth_case(m, 4, 19, B=B, S=S, rbar=1.5)
    e = staged(m, sp, R * K)
    try:
        q = m["cluster"].hwe_prior(np.zeros(S), np.zeros(S))
        e.cluster_mstep(rng.random((B, R * K)), q, fetch=False)
        e.set_genotypes_device(e.cluster_device_ptr(), S)
        e.run_singlet()
        llks, _ = e.get_singlet()
        log_pi = np.log(rng.dirichlet(np.ones(K), size=R))
        group = rng.integers(-1, R // Rs, size=B).astype(np.int32)
        mask = rng.random(B) < 0.8
        for T, mk in ((1.0, None), (1.0, mask), (2.0, mask)):
            ll, cs = e.cluster_estep_grouped(R, K, log_pi, group, Rs, T, mk)
            w = e.cluster_weights()
            rw, rll, rcs = SM.estep_grouped(llks, R, K, log_pi, group, Rs, T, mk)
            assert np.allclose(w, rw, rtol=1e-12, atol=1e-290)
            assert np.allclose(ll, rll, rtol=1e-12, atol=0) and np.allclose(cs, rcs, rtol=1e-12, atol=1e-12)
            inside = group[:, None] == (np.arange(R) // Rs)[None, :]
            assert not w.reshape(B, R, K)[~inside].any()
        # one group with every barcode and restarts_per_group = R: cluster_estep bit for bit
        ll_g, cs_g = e.cluster_estep_grouped(R, K, log_pi, np.zeros(B, dtype=np.int32), R, 1.0, mask)
        w_g = e.cluster_weights()
        ll_p, cs_p = e.cluster_estep(R, K, log_pi, 1.0, mask)
        w_p = e.cluster_weights()
        assert np.array_equal(bits(w_g), bits(w_p)) and np.array_equal(bits(ll_g), bits(ll_p)) and np.array_equal(bits(cs_g), bits(cs_p))
    finally:
        e.close()


def planted_labels(truth, seed):
    """truth's donors as clusters, except donors 0 and 1 share cluster 0 and donor 2 is split at random into clusters 1 and 2."""
    d = truth[:, 0].astype(np.int64)
    lab = d.copy()
    lab[d == 1] = 0
    two = np.flatnonzero(d == 2)
    lab[two] = 1 + np.random.default_rng(seed).integers(0, 2, size=two.size)
    return lab[None, :].astype(np.int32)


# measured on an MI355X: see DESIGN.md section 16
# With 10 % doublets and no doublet components, plain EM from the planted start turns one half of donor 2 into a sink of doublets: the
# pair to merge is then that cluster and another, not (1, 2); the split is still cluster 0.
@pytest.mark.parametrize("doublets,rate,first", [(False, 0.0, (1, 2, 0)), (False, 0.1, (None, None, 0)), (True, 0.25, (1, 2, 0))])
def test_planted_local_optimum(m, tmp_path, doublets, rate, first):
    K = 8
    raw, sp, pl, barcodes = synth_case(m, K, 808 if doublets else 202, doublet_rate=rate)
    init = planted_labels(sp.truth, 1)
    run = m["cluster"].cluster_run
    run(pl, K, str(tmp_path / "p"), barcodes=barcodes, init_labels=init, em_doublets=doublets)
    plain = accuracy(m, sp.truth, barcodes, str(tmp_path / "p"), K)
    res = run(pl, K, str(tmp_path / "s"), barcodes=barcodes, init_labels=init, em_doublets=doublets, split_merge=True)
    sm = accuracy(m, sp.truth, barcodes, str(tmp_path / "s"), K)
    acc = [r for r in res["moves"] if r["accepted"]]
    print(f"planted K=8 doublets={doublets} rate={rate}: plain singlets {plain[0]:.4f} doublets {plain[1]:.4f}; split-merge singlets {sm[0]:.4f}"
          f" doublets {sm[1]:.4f}; {len(acc)} moves accepted: " + ", ".join(f"({r['merge_k']},{r['merge_l']})+{r['split']}" for r in acc))
    for r in res["moves"]:
        print(f"  move {r['move']} cand {r['cand']}: merge ({r['merge_k']},{r['merge_l']}) BF {r['bf']:.1f}, split {r['split']} gain"
              f" {r['gain']:.1f}: LL {r['ll_before']:.3f} -> {r['ll_after']:.3f} in {r['iterations']} iterations{' ACCEPTED' if r['accepted'] else ''}")
    assert plain[0] < 0.95                                 # the start is a real local optimum of plain EM
    assert sm[0] >= 0.99
    if doublets:
        assert sm[1] >= 0.95
    assert acc and acc[0]["split"] == first[2]
    if first[0] is not None:
        assert (acc[0]["merge_k"], acc[0]["merge_l"]) == first[:2]
    rows = (tmp_path / "s.moves.tsv").read_text().splitlines()
    assert len(rows) == 1 + len(res["moves"]) and not (tmp_path / "p.moves.tsv").exists()


def test_single_restarts_k8(m, tmp_path):
    K = 8
    raw, sp, pl, barcodes = synth_case(m, K, 202)
    out = []
    for seed in range(6):
        pre = str(tmp_path / f"s{seed}")
        res = m["cluster"].cluster_run(pl, K, pre, restarts=1, seed=seed, barcodes=barcodes, split_merge=True)
        a = accuracy(m, sp.truth, barcodes, pre, K)
        out.append(a[0])
        print(f"K=8 restarts=1 seed {seed}: singlets {a[0]:.4f}, {sum(r['accepted'] for r in res['moves'])} moves accepted")
    assert sum(x >= 0.95 for x in out) >= 5, out


def test_full_size_cfg6_shape(m, tmp_path):
    """The data and seed of tests/test_gpu_cluster.py::test_full_size_cfg6_shape, with split_merge=True."""
    torch = m["torch"]
    from demuxlet_amd import synth_torch
    K, B, S = 16, 20_000, 100_000
    rng = np.random.default_rng(0xC1)
    raw = m["synth"].make_raw_genotypes(rng, S, K)
    dev = torch.device("cuda", 0)
    dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
    dp = synth_torch.make_device_pileup(dosage, B, 0.02, 1.25, seed=0xC1C1, device=dev)
    h = dp.host_slice(0, B)
    truth = dp.truth.cpu().numpy()
    z = np.zeros(B, dtype=np.int32)
    pl = m["engine"].HostPileup(rd_totl=z, rd_pass=z, rd_uniq=z, **h)
    del dp, dosage
    barcodes = [m["synth"].barcode_name(c) for c in range(B)]
    t0 = time.perf_counter()
    res = m["cluster"].cluster_run(pl, K, str(tmp_path / "f"), restarts=4, seed=1, barcodes=barcodes, split_merge=True)
    wall = time.perf_counter() - t0
    sng, dbl, per = accuracy(m, truth, barcodes, str(tmp_path / "f"), K)
    acc = [r for r in res["moves"] if r["accepted"]]
    print(f"cfg6 shape K=16 split-merge: wall {wall:.1f} s, iterations {res['iterations']}, {len(res['moves'])} candidates, {len(acc)} moves"
          f" accepted, singlets {sng:.4f}, doublets {dbl:.4f}, worst donor {per.min():.4f}")
    assert sng >= 0.99 and (per >= 0.95).all()
    assert wall < 60.0


def test_no_op_when_em_is_right(m, tmp_path):
    K = 4
    raw, sp, pl, barcodes = synth_case(m, K, 101)
    run = m["cluster"].cluster_run
    run(pl, K, str(tmp_path / "a"), seed=101, barcodes=barcodes)
    r1 = run(pl, K, str(tmp_path / "b"), seed=101, barcodes=barcodes, split_merge=True)
    run(pl, K, str(tmp_path / "c"), seed=101, barcodes=barcodes, split_merge=True)
    assert r1["moves"] and not any(r["accepted"] for r in r1["moves"])
    for ext in (".best", ".single", ".sing2", ".r1.best", ".r1.single", ".r1.sing2", ".em.tsv", ".clust.tsv"):
        assert (tmp_path / ("a" + ext)).read_bytes() == (tmp_path / ("b" + ext)).read_bytes(), ext
    outs = sorted(p.name[1:] for p in tmp_path.iterdir() if p.name.startswith("b."))
    assert ".moves.tsv" in outs and outs == sorted(p.name[1:] for p in tmp_path.iterdir() if p.name.startswith("c."))
    for ext in outs:
        assert (tmp_path / ("b" + ext)).read_bytes() == (tmp_path / ("c" + ext)).read_bytes(), ext


def test_k2_equals_plain_run(m, tmp_path):
    raw, sp, pl, barcodes = synth_case(m, 2, 55, B=600, S=3000)
    run = m["cluster"].cluster_run
    run(pl, 2, str(tmp_path / "a"), restarts=2, seed=3, barcodes=barcodes)
    res = run(pl, 2, str(tmp_path / "b"), restarts=2, seed=3, barcodes=barcodes, split_merge=True)
    assert res["moves"] == []
    for ext in (".best", ".single", ".sing2", ".r1.best", ".em.tsv", ".clust.tsv"):
        assert (tmp_path / ("a" + ext)).read_bytes() == (tmp_path / ("b" + ext)).read_bytes(), ext
    assert (tmp_path / "b.moves.tsv").read_text() == m["cluster"].MOVES_HEADER


def test_cli_split_merge(m, tmp_path):
    raw, sp, pl, barcodes = synth_case(m, 3, 404, B=600, S=3000)
    g = np.stack([m["engine"].geno_from_gt(raw.alleles[s], 0.01) for s in range(sp.n_snps)])
    d = m["refine"].PileupDump([f"s{v}" for v in range(3)], [(1, 100 + s, "A", "G") for s in range(sp.n_snps)], g, barcodes, pl)
    p = tmp_path / "x.pileup.txt"
    m["refine"].write_pileup_txt(str(p), d)
    assert m["cluster"].main(["--pileup", str(p), "--n-clusters", "3", "--out", str(tmp_path / "c"), "--restarts", "2", "--split-merge"]) == 0
    for ext in (".best", ".single", ".sing2", ".r1.best", ".em.tsv", ".clust.tsv", ".moves.tsv"):
        assert (tmp_path / ("c" + ext)).stat().st_size > 0, ext
    assert (tmp_path / "c.moves.tsv").read_text().startswith(m["cluster"].MOVES_HEADER)
