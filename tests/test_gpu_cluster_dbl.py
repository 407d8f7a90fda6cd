"""GPU (-m gpu): doublet-aware clustering (Engine.cluster_doublet / cluster_estep_doublet, cluster.cluster_run(em_doublets=True);
DESIGN.md section 15).

LLD is checked against the float64 restatement (tests/cluster_dbl_ref.py), the oracle's llksAB at alpha = 0.5 and the engine's own
STRICT grid (1e-9), over dense and sparse layouts, u16 read counts, pairs without stored reads, barcodes without pairs, GT / GP / PL
matrices and K from 2 to 40 with R > 1.  Then: a restart's bits do not depend on R or on its place, repeated calls give the same
bits, the doublet E-step against the restatement (1e-12 relative) and against the plain E-step at delta = 0, the error paths, no
interference with the engine's other results, recovery against the plain EM at a 25 % doublet rate, a cfg6-shaped run and the
command line."""
import time

import numpy as np
import pytest

import cluster_dbl_ref as D

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


def genotypes(m, rng, alleles, kind):
    eng, syn = m["engine"], m["synth"]
    S = alleles.shape[0]
    if kind == "GT":
        return np.stack([eng.geno_from_gt(alleles[s], 0.01) for s in range(S)])
    if kind == "GP":
        gp = syn.raw_gp_from_alleles(rng, alleles, soft=0.3)
        return np.stack([eng.geno_from_gp(gp[s], 0.01) for s in range(S)])
    pl = syn.raw_pl_from_alleles(rng, alleles)
    return np.stack([eng.geno_from_pl(pl[s]) for s in range(S)])


def oracle_llksAB(O, sp, g):
    """The oracle's llksAB[B][V][V][A] on the grid {0, 0.5}."""
    B = sp.n_cells
    po = np.asarray(sp.cell_pair_off, dtype=np.int64)
    snp = sp.pair_snp if sp.pair_snp is not None else (np.arange(po[-1]) - np.repeat(po[:-1], np.diff(po))).astype(np.int32)
    reads = np.asarray(sp.reads)
    words = ((reads >> 7).astype(np.uint32) << 24) | ((reads & 0x7F).astype(np.uint32) << 16) | 1
    csr = O.Csr([f"c{i}" for i in range(B)], sp.cell_pair_off, snp, np.concatenate([[0], np.cumsum(sp.pair_nrd.astype(np.int64))]),
                words.astype(np.uint32), sp.rd_totl, sp.rd_pass, sp.rd_uniq)
    return O.run_csr(csr, [f"s{j}" for j in range(g.shape[1])], g, O.Params((0.0, 0.5), 0.5)).llksAB


def lld_from_grid(grid, R, K):
    """LLD[B][R][P] picked from a grid [B][V][V][A] at alpha index 1 (0.5): llksAB[b][rK + k][rK + l]."""
    pr = D.pairs(K)
    return np.stack([grid[:, r * K + pr[:, 0], r * K + pr[:, 1], 1] for r in range(R)], axis=1)


@pytest.mark.parametrize("S,B,delta,rbar,dense,R,K,kind", [
    (400, 40, 0.3, 1.5, False, 2, 5, "GT"),       # sparse, R > 1
    (150, 30, 1.0, 1.25, True, 1, 12, "GP"),      # dense; P = 66 crosses a 64-lane block
    (60, 12, 0.4, 300.0, False, 1, 3, "PL"),      # u16 read counts
    (700, 60, 0.3, 1.0, False, 3, 4, "GT"),       # one read per pair: many pairs whose reads are all allele 2 (none stored)
    (400, 80, 0.0005, 1.5, False, 2, 3, "GP"),    # most barcodes have no pair
    (200, 16, 0.3, 1.5, False, 2, 40, "GT"),      # K = 40: P = 780, 1 560 pair-columns in 25 blocks
    (120, 20, 0.5, 1.5, False, 3, 2, "PL"),       # K = 2: one pair per restart
])
def test_lld_parity(m, oracle, S, B, delta, rbar, dense, R, K, kind):
    rng = np.random.default_rng(S * 7 + B + K)
    V = R * K
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, delta, rbar, dense_layout=dense)
    assert (sp.pair_snp is None) == dense
    npc = np.diff(sp.cell_pair_off)
    if rbar > 100:
        assert sp.pair_nrd.dtype == np.uint16 and int(sp.pair_nrd.max()) > 255
    if rbar == 1.0:
        assert (np.asarray(sp.pair_nrd) == 0).any()
    if delta < 0.01:
        assert (npc == 0).sum() > B // 2
    g = genotypes(m, rng, raw.alleles, kind)
    e = m["engine"].Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g)
        e.set_pileup(host_pileup(m, sp))
        e.cluster_doublet(R, K)
        lld, lsc = e.get_cluster_doublet()
        inf = e.cluster_doublet_info()
        e.run_doublet()
        grid = e.get_cell_grids(np.arange(B))
    finally:
        e.close()
    P = K * (K - 1) // 2
    assert lld.shape == (B, R, P)
    assert inf["n_pairs"] == P and inf["n_restarts"] == R and inf["n_clusters"] == K and inf["lld_bytes"] == 8 * B * (R * P + 1)
    mat, err = m["engine"].phred_tables()
    ref, rsc = D.lld(sp, g, R, K, mat, err)
    assert np.abs(lld - ref).max() <= 1e-9, np.abs(lld - ref).max()
    assert np.abs(lsc - rsc).max() <= 1e-9, np.abs(lsc - rsc).max()
    assert not lld[npc == 0].any() and not lsc[npc == 0].any()
    has = npc > 0
    o = lld_from_grid(oracle_llksAB(oracle, sp, g), R, K)
    assert np.abs(lld[has] - o[has]).max() <= 1e-9
    s = lld_from_grid(grid, R, K)
    assert np.abs(lld[has] - s[has]).max() <= 1e-9


def test_restart_independence_and_determinism(m):
    """Restart 2 of R = 4 with the same columns as a lone restart gives the same bits; repeated calls too."""
    rng = np.random.default_rng(77)
    S, B, K = 2000, 300, 9
    raw = m["synth"].make_raw_genotypes(rng, S, 4 * K)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.2, 1.5)
    g4 = genotypes(m, rng, raw.alleles, "GP")
    g1 = np.ascontiguousarray(g4[:, 2 * K:3 * K])
    pl = host_pileup(m, sp)
    out = {}
    for R, g in ((1, g1), (4, g4)):
        e = m["engine"].Engine(R * K, (0.0, 0.5), 0.5)
        try:
            e.set_genotypes(g); e.set_pileup(pl)
            e.cluster_doublet(R, K)
            a, sa = e.get_cluster_doublet()
            e.cluster_doublet(R, K)
            b, sb = e.get_cluster_doublet()
        finally:
            e.close()
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.array_equal(sa.view(np.uint64), sb.view(np.uint64))
        out[R] = a, sa
    assert np.array_equal(out[1][0][:, 0].view(np.uint64), out[4][0][:, 2].view(np.uint64))
    assert np.array_equal(out[1][1].view(np.uint64), out[4][1].view(np.uint64))


def staged(m, sp, g):
    e = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    e.set_genotypes(g)
    e.set_pileup(host_pileup(m, sp))
    e.cluster_stage()
    return e


def test_estep_parity(m):
    rng = np.random.default_rng(91)
    S, B, R, K = 1500, 500, 3, 5
    C = R * K
    raw = m["synth"].make_raw_genotypes(rng, S, C)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.1, 1.5, doublet_rate=0.25)
    g = genotypes(m, rng, raw.alleles, "GP")
    e = staged(m, sp, g)
    try:
        e.run_singlet()
        llks, _ = e.get_singlet()
        e.cluster_doublet(R, K)
        lld, lsc = e.get_cluster_doublet()
        lld = lld - lsc[:, None, None]
        log_pi = np.log(rng.dirichlet(np.ones(K), size=R))
        mask = rng.random(B) < 0.8
        for T, mk, delta in ((1.0, None, [0.1, 0.25, 0.4]), (1.0, mask, [0.05, 0.1, 0.2]), (2.5, mask, [0.3, 0.001, 0.5])):
            ld = np.log(delta)
            ll, cs, dbl = e.cluster_estep_doublet(R, K, log_pi, ld, T, mk)
            w = e.cluster_weights()
            rw, rdm, rll, rcs, rdbl = D.estep(llks, lld, log_pi, ld, T, mk)
            assert np.allclose(w, rw, rtol=1e-12, atol=1e-290)
            assert np.allclose(ll, rll, rtol=1e-12, atol=0)
            assert np.allclose(cs, rcs, rtol=1e-12, atol=1e-12)
            assert np.allclose(dbl, rdbl, rtol=1e-12, atol=1e-12)
            keep = np.ones(B, bool) if mk is None else mk
            assert not w[~keep].any() and (dbl > 0).all()
        # delta = 0: the plain E-step's results
        for T, mk in ((1.0, None), (2.5, mask)):
            ll, cs, dbl = e.cluster_estep_doublet(R, K, log_pi, np.full(R, -np.inf), T, mk)
            w = e.cluster_weights()
            pll, pcs = e.cluster_estep(R, K, log_pi, T, mk)
            pw = e.cluster_weights()
            assert not dbl.any()
            assert np.allclose(w, pw, rtol=1e-12, atol=1e-290) and np.allclose(ll, pll, rtol=1e-12, atol=0)
            assert np.allclose(cs, pcs, rtol=1e-12, atol=1e-12)
        # the doublet E-step's weights feed the M-step
        e.cluster_estep_doublet(R, K, log_pi, np.log([0.1, 0.2, 0.3]))
        w = e.cluster_weights()
        q = m["cluster"].hwe_prior(np.zeros(S), np.zeros(S))
        a = e.cluster_mstep(None, q)
        b = e.cluster_mstep(w, q)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    finally:
        e.close()


def test_error_paths(m):
    capi = m["capi"]
    rng = np.random.default_rng(5)
    S, B = 300, 50
    raw = m["synth"].make_raw_genotypes(rng, S, 6)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.2, 1.5)
    g = genotypes(m, rng, raw.alleles, "GT")
    e = m["engine"].Engine(6, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(host_pileup(m, sp))

        def code(f, *a):
            with pytest.raises(capi.DmxError) as ei:
                f(*a)
            return ei.value.code
        assert code(e.get_cluster_doublet) == capi.DMX_ERR_STATE
        assert code(e.cluster_doublet_info) == capi.DMX_ERR_STATE
        assert code(e.cluster_doublet, 6, 1) == capi.DMX_ERR_ARG          # K < 2
        assert code(e.cluster_doublet, 2, 2) == capi.DMX_ERR_ARG          # R * K != V
        assert code(e.cluster_doublet, 0, 6) == capi.DMX_ERR_ARG
        e.cluster_stage()
        e.run_singlet()
        lp = np.full((2, 3), -np.log(3))
        assert code(e.cluster_estep_doublet, 2, 3, lp, np.log([0.1, 0.1])) == capi.DMX_ERR_STATE   # no LLD yet
        e.cluster_doublet(2, 3)
        assert code(e.cluster_estep_doublet, 3, 2, np.full((3, 2), -np.log(2)), np.log([0.1] * 3)) == capi.DMX_ERR_STATE   # other R, K
        assert code(e.cluster_estep_doublet, 2, 3, lp, np.array([0.0, -1.0])) == capi.DMX_ERR_ARG  # delta = 1
        assert code(e.cluster_estep_doublet, 2, 3, lp, np.array([np.nan, -1.0])) == capi.DMX_ERR_ARG
        e.cluster_estep_doublet(2, 3, lp, np.log([0.1, 0.1]))
        e.set_pileup(host_pileup(m, sp))                                   # staging again drops LLD
        assert code(e.get_cluster_doublet) == capi.DMX_ERR_STATE
    finally:
        e.close()


def test_no_interference(m):
    eng = m["engine"]
    rng = np.random.default_rng(29)
    S, V, B = 800, 8, 300
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.2, 1.5)
    g = genotypes(m, rng, raw.alleles, "GT")
    pl = host_pileup(m, sp)
    q = m["cluster"].hwe_prior(np.zeros(S), np.zeros(S))
    assign = rng.integers(-1, V, size=B).astype(np.int32)
    prior = np.ascontiguousarray(np.broadcast_to(q[:, None, :], (S, V, 3)))

    def results(e):
        llks, llk0s = e.get_singlet()
        grid, l00, summ = e.get_doublet()
        return [llks, llk0s, grid, l00, summ.view(np.uint8)]

    def run(with_dbl):
        e = eng.Engine(V, (0.0, 0.5), 0.5)
        try:
            e.set_genotypes(g); e.set_pileup(pl)
            e.cluster_stage()
            stage0 = e.get_cluster_stage()
            if with_dbl:
                e.cluster_doublet(2, 4)
            e.run_singlet()
            if with_dbl:
                e.cluster_estep_doublet(2, 4, np.full((2, 4), -np.log(4)), np.log([0.1, 0.2]))
            ll, cs = e.cluster_estep(2, 4, np.full((2, 4), -np.log(4)))
            w = e.cluster_weights()
            mst = e.cluster_mstep(None, q)
            ref = e.refine_genotypes(assign, prior, 1e-3)
            e.run(); e.sync()
            stage1 = e.get_cluster_stage()
            return [*results(e), ll, cs, w, *mst, *ref, *stage0, *stage1]
        finally:
            e.close()
    base, after = run(False), run(True)
    assert len(base) == len(after)
    for x, y in zip(base, after):
        x, y = np.asarray(x), np.asarray(y)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def read_best(path):
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        col = {n: i for i, n in enumerate(head)}
        return {t[col["BARCODE"]]: t[col["BEST"]] for t in (ln.rstrip("\n").split("\t") for ln in f)}


def accuracy(m, truth, barcodes, prefix, K):
    """(share of true singlets called SNG- of the right cluster, share of true doublets called DBL-, cluster -> donor map), after
    greedy label matching (tests/test_gpu_cluster.py's measure)."""
    best = read_best(prefix + ".best")
    calls = [best.get(b, "") for b in barcodes]
    sng = np.array([int(c[len("SNG-CLUST"):]) if c.startswith("SNG-") else -1 for c in calls])
    is_dbl = np.array([c.startswith("DBL-") for c in calls])
    truth_s = np.where(truth[:, 1] < 0, truth[:, 0], -1)
    lab = m["cluster"].match_labels(truth_s, sng, K, K)
    mapped = np.where(sng >= 0, lab[np.maximum(sng, 0)], -1)
    singlet = truth[:, 1] < 0
    return float((mapped[singlet] == truth[singlet, 0]).mean()), float(is_dbl[~singlet].mean()), lab


def genotype_error(gp, lab, dosage, cell_pair_off, pair_snp, truth, K, min_cells=3):
    """Share of (SNP, cluster) rows whose argmax genotype is not the matched donor's, over SNPs with >= min_cells covering true
    singlets of that donor."""
    po = np.asarray(cell_pair_off, dtype=np.int64)
    cell = np.repeat(np.arange(len(po) - 1), np.diff(po))
    sng = truth[cell, 1] < 0
    S = dosage.shape[0]
    cov = np.zeros((S, dosage.shape[1]), dtype=np.int64)
    np.add.at(cov, (np.asarray(pair_snp)[sng], truth[cell[sng], 0]), 1)
    bad = tot = 0
    for k in range(K):
        v = lab[k]
        if v < 0:
            continue
        rows = cov[:, v] >= min_cells
        call = gp[rows, k, :].argmax(axis=1)
        bad += int((call != dosage[rows, v]).sum())
        tot += int(rows.sum())
    return bad / max(tot, 1), tot


# measured on an MI355X (K = 8, 4 000 barcodes, ~1 000 covered SNPs each, 25 % doublets (0.243 realised), 16 restarts, seed 808):
# plain EM 0.8804 of the singlets right, 0.9558 of the doublets DBL-, genotype error 0.0993; em_doublets 1.0000 / 1.0000 / 0.0000 with
# delta 0.2430.  Thresholds: never worse than the plain EM, and absolute floors with margin
def test_recovery_against_plain_em(m, tmp_path):
    K, B, S, seed = 8, 4000, 10000, 808
    rng = np.random.default_rng(seed)
    raw = m["synth"].make_raw_genotypes(rng, S, K)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.1, 1.25, doublet_rate=0.25)
    npc = np.diff(sp.cell_pair_off)
    share = float((sp.truth[:, 1] >= 0).mean())
    assert 800 <= npc.mean() <= 1200 and 0.22 <= share <= 0.28
    pl = host_pileup(m, sp)
    barcodes = [m["synth"].barcode_name(c) for c in range(B)]
    dosage = np.clip(raw.alleles, 0, 1).sum(axis=2)
    figs = {}
    for name, flag in (("plain", False), ("dbl", True)):
        pre = str(tmp_path / name)
        t0 = time.perf_counter()
        res = m["cluster"].cluster_run(pl, K, pre, seed=seed, barcodes=barcodes, em_doublets=flag)
        wall = time.perf_counter() - t0
        acc = accuracy(m, sp.truth, barcodes, pre, K)
        gerr, n_rows = genotype_error(res["gp"], acc[2], dosage, sp.cell_pair_off, sp.pair_snp, sp.truth, K)
        figs[name] = (acc[0], acc[1], gerr, res)
        print(f"{name}: singlets {acc[0]:.4f} doublets {acc[1]:.4f} genotype error {gerr:.5f} ({n_rows} rows) iterations {res['iterations']}"
              f" delta {res.get('delta', float('nan')):.4f} (true share {share:.4f}) wall {wall:.1f} s")
        assert ("delta" in res) == flag
    em = (tmp_path / "dbl.em.tsv").read_text().splitlines()
    assert em[0] == "ITER\tRESTART\tLLK\tPI\tDBL" and len(em) == 1 + 16 * figs["dbl"][3]["iterations"]
    assert (tmp_path / "plain.em.tsv").read_text().splitlines()[0] == "ITER\tRESTART\tLLK\tPI"
    assert abs(figs["dbl"][3]["delta"] - share) <= 0.05
    assert figs["dbl"][0] >= figs["plain"][0] and figs["dbl"][1] >= figs["plain"][1]
    assert figs["dbl"][2] <= figs["plain"][2]
    assert figs["dbl"][0] >= 0.95 and figs["dbl"][1] >= 0.7


# measured on an MI355X: 5.6 s, 50 iterations, 0.9366 of the singlets right, 0.9907 of the doublets DBL-, delta 0.0959 (true 0.0968)
def test_full_size_cfg6_shape(m, tmp_path):
    """20 000 barcodes x 100 000 SNPs, ~2 000 covered SNPs per barcode (cfg6's shape), K = 16, R = 4, with doublet components."""
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
    res = m["cluster"].cluster_run(pl, K, str(tmp_path / "f"), restarts=4, seed=1, barcodes=barcodes, em_doublets=True)
    wall = time.perf_counter() - t0
    acc = accuracy(m, truth, barcodes, str(tmp_path / "f"), K)
    share = float((truth[:, 1] >= 0).mean())
    print(f"cfg6 shape K=16 with doublet components: wall {wall:.1f} s, iterations {res['iterations']}, singlets {acc[0]:.4f},"
          f" doublets {acc[1]:.4f}, delta {res['delta']:.4f} (true share {share:.4f})")
    assert acc[0] >= 0.85 and acc[1] >= 0.85
    assert abs(res["delta"] - share) <= 0.05
    assert wall < 120.0


def test_cli_on_pileup_dump(m, tmp_path):
    rng = np.random.default_rng(404)
    S, B, K = 3000, 600, 3
    raw = m["synth"].make_raw_genotypes(rng, S, K)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.1, 1.25)
    g = genotypes(m, rng, raw.alleles, "GT")
    barcodes = [m["synth"].barcode_name(c) for c in range(B)]
    d = m["refine"].PileupDump([f"s{v}" for v in range(K)], [(1, 100 + s, "A", "G") for s in range(S)], g, barcodes, host_pileup(m, sp))
    p = tmp_path / "x.pileup.txt"
    m["refine"].write_pileup_txt(str(p), d)
    assert m["cluster"].main(["--pileup", str(p), "--n-clusters", "3", "--out", str(tmp_path / "c"), "--restarts", "2", "--em-doublets"]) == 0
    for ext in (".best", ".single", ".sing2", ".r1.best", ".em.tsv", ".clust.tsv"):
        assert (tmp_path / ("c" + ext)).stat().st_size > 0, ext
    em = (tmp_path / "c.em.tsv").read_text().splitlines()
    assert em[0] == "ITER\tRESTART\tLLK\tPI\tDBL"
    assert all(len(ln.split("\t")) == 5 and 1e-3 <= float(ln.split("\t")[4]) <= 0.5 for ln in em[1:])
    acc = accuracy(m, sp.truth, barcodes, str(tmp_path / "c"), 3)
    assert acc[0] >= 0.9


@pytest.mark.parametrize("quals", ["full", "edges", "max"])
@pytest.mark.parametrize("R,K,kind,dense", [(2, 5, "GT", False), (1, 12, "GP", True), (3, 3, "PL", False)])
def test_lld_parity_quality_range(m, oracle, R, K, kind, dense, quals):
    """k_cluster_dbl's LLD against cluster_dbl_ref and the oracle's llksAB on reads of quality 0..127 and the depth mix of
    tests/quality_mix.py (0..6, 14..17, 40, u16 pairs of 256..300 reads, all-ALT pairs on hom-REF rows)."""
    from quality_mix import mixed_depth_pileup
    rng = np.random.default_rng(4400 + R * K + {"full": 0, "edges": 1, "max": 2}[quals])
    V = R * K
    S, B = (90, 20) if dense else (300, 40)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    sp = mixed_depth_pileup(rng, raw.alleles, B, 0.3, quals=quals, dense=dense, deep=0 if dense else 3)
    g = genotypes(m, rng, raw.alleles, kind)
    e = m["engine"].Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g)
        e.set_pileup(host_pileup(m, sp))
        e.cluster_doublet(R, K)
        lld, lsc = e.get_cluster_doublet()
    finally:
        e.close()
    mat, err = m["engine"].phred_tables()
    ref, rsc = D.lld(sp, g, R, K, mat, err)
    assert np.abs(lld - ref).max() <= 1e-9, np.abs(lld - ref).max()
    assert np.abs(lsc - rsc).max() <= 1e-9, np.abs(lsc - rsc).max()
    has = np.diff(sp.cell_pair_off) > 0
    o = lld_from_grid(oracle_llksAB(oracle, sp, g), R, K)
    assert np.abs(lld[has] - o[has]).max() <= 1e-9
