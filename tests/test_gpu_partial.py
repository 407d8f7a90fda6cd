"""GPU (-m gpu): partly genotyped pools (Engine.cluster_estep_known / cluster_mstep_window, partial.partial_run).

The known-column E-step is checked against the float64 restatement in partial_ref.py (1e-12 relative) and, with no known columns, bit
for bit against cluster_estep; the windowed M-step against the restatement (LL 1e-9, W 1e-12, gp' 2 float32 ulp, the known columns the
input's bits in both buffers) and, with no known columns, bit for bit against cluster_mstep.  Then determinism, no interference with the
engine's other results, recovery of dropped donors on synthetic pools (sparse and dense, M = 1 and 2, M too large), the cfg6 shape
and the CLI."""
import time

import numpy as np
import pytest

import partial_ref as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import build, capi, cluster, engine, partial, refine, synth
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return dict(torch=torch, capi=capi, cluster=cluster, engine=engine, partial=partial, refine=refine, synth=synth)


def host_pileup(m, sp):
    return m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads,
                                  sp.rd_totl, sp.rd_pass, sp.rd_uniq)


def make_sp(m, rng, S, V, B, delta, rbar, dense=False, doublet_rate=0.1):
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    return raw, m["synth"].make_pileup(rng, raw.alleles, B, delta, rbar, dense_layout=dense, doublet_rate=doublet_rate)


def soft_g(m, rng, S, C):
    g = m["synth"].raw_gp_from_alleles(rng, m["synth"].make_raw_genotypes(rng, S, C).alleles, soft=0.3)
    return np.stack([m["engine"].geno_from_gp(g[s], 0.01) for s in range(S)])


def staged(m, sp, C, g=None):
    e = m["engine"].Engine(C, (0.0, 0.5), 0.5)
    e.set_genotypes(np.full((sp.n_snps, C, 3), 1 / 3, dtype=np.float32) if g is None else g)
    e.set_pileup(host_pileup(m, sp))
    e.cluster_stage()
    return e


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


@pytest.mark.parametrize("Vk", [1, 7, 64])
@pytest.mark.parametrize("M", [1, 3])
def test_estep_known_parity(m, Vk, M):
    rng = np.random.default_rng(100 * Vk + M)
    S, B, R = 600, 700, 3                      # 700 barcodes: three chunks of 256, the last one ragged
    V = Vk + R * M
    _, sp = make_sp(m, rng, S, 4, B, 0.1, 1.5)
    e = staged(m, sp, V, soft_g(m, rng, S, V))
    try:
        e.run_singlet()
        llks, _ = e.get_singlet()
        log_pi = np.log(rng.dirichlet(np.ones(Vk + M), size=R))
        mask = rng.random(B) < 0.8
        for T, mk in ((1.0, None), (1.0, mask), (2.5, mask)):
            ll, cs = e.cluster_estep_known(R, Vk, M, log_pi, T, mk)
            wk, wf = e.cluster_known_weights()
            rwk, rwf, rll, rcs = PR.estep_known(llks, R, Vk, M, log_pi, T, mk)
            assert np.allclose(wk, rwk, rtol=1e-12, atol=1e-290)
            assert np.array_equal(wf, np.ascontiguousarray(wk[:, :, Vk:]).reshape(B, R * M))
            assert np.allclose(ll, rll, rtol=1e-12, atol=0)
            assert np.allclose(cs, rcs, rtol=1e-12, atol=1e-12)
            if mk is not None:
                assert not wk[~mk].any()
        assert e.cluster_known_info()["estep_ms"] > 0
    finally:
        e.close()


@pytest.mark.parametrize("dense", [False, True])
def test_no_known_columns_equal_the_clustering_calls(m, dense):
    """Vk = 0: the E-step gives cluster_estep's bits (weights, LL, column sums) and the windowed M-step cluster_mstep's."""
    rng = np.random.default_rng(7 + dense)
    S, B, R, M = (900, 555, 4, 3) if not dense else (300, 300, 4, 3)
    C = R * M
    _, sp = make_sp(m, rng, S, 4, B, 1.0 if dense else 0.1, 1.5, dense)
    q = m["cluster"].hwe_prior(rng.integers(0, 20, S), rng.integers(0, 20, S))
    e = staged(m, sp, C, soft_g(m, rng, S, C))
    try:
        e.run_singlet()
        log_pi = np.log(rng.dirichlet(np.ones(M), size=R))
        mask = rng.random(B) < 0.9
        for T, mk in ((1.0, None), (1.7, mask)):
            ll_a, cs_a = e.cluster_estep(R, M, log_pi, T, mk)
            w_a = e.cluster_weights()
            LL_a, W_a, gp_a = e.cluster_mstep(None, q, 1e-3)
            ll_b, cs_b = e.cluster_estep_known(R, 0, M, log_pi, T, mk)
            wk, w_b = e.cluster_known_weights()
            e.cluster_set_known(np.zeros((S, 0, 3), dtype=np.float32))
            LL_b, W_b, gp_b = e.cluster_mstep_window(None, R, M, q, 1e-3)
            for x, y in ((ll_a, ll_b), (cs_a, cs_b.reshape(-1)), (w_a, w_b), (w_a, wk.reshape(B, C)), (LL_a, LL_b), (W_a, W_b), (gp_a, gp_b)):
                assert same_bits(x, y)
        w = rng.dirichlet(np.ones(C), size=B)
        for x, y in zip(e.cluster_mstep(w, q, 1e-3), e.cluster_mstep_window(w, R, M, q, 1e-3)):
            assert same_bits(x, y)
    finally:
        e.close()


@pytest.mark.parametrize("S,B,delta,Vk,R,M,dense", [(2000, 300, 0.2, 5, 4, 16, False), (257, 150, 1.0, 3, 2, 1, True),
                                                     (900, 64, 0.05, 64, 3, 3, False)])
def test_mstep_window_parity(m, S, B, delta, Vk, R, M, dense):
    rng = np.random.default_rng(S + Vk)
    C = R * M
    V = Vk + C
    _, sp = make_sp(m, rng, S, 4, B, delta, 1.5, dense)
    w = rng.dirichlet(np.ones(C), size=B) * rng.random((B, 1))
    w[:, C - 1] = 0.0                                        # a column without weight: every row is q's
    w[rng.random(B) < 0.2] = 0.0
    q = m["cluster"].hwe_prior(rng.integers(0, 20, S), rng.integers(0, 20, S))
    gk = soft_g(m, rng, S, Vk)
    e = staged(m, sp, V)
    try:
        with pytest.raises(m["capi"].DmxError, match="known rows"):
            e.cluster_mstep_window(w, R, M, q)                # DMX_ERR_STATE before the known rows
        e.cluster_set_known(gk)
        with pytest.raises(m["capi"].DmxError, match="columns"):
            e.cluster_mstep_window(np.zeros((B, C + M)), R + 1, M, q)     # Vk + R M != V
        off, cell, lgl = e.get_cluster_stage()[:3]
        LL, W, gp = e.cluster_mstep_window(w, R, M, q, 1e-3)
        ptrs = {e.cluster_device_ptr()}
        # several iterations through K1: the M-step writes the other buffer each time, and both keep the known rows' bits
        for _ in range(3):
            e.set_genotypes_device(e.cluster_device_ptr(), S)
            if dense:
                e.set_pileup(host_pileup(m, sp))
            again = e.cluster_mstep_window(w, R, M, q, 1e-3)
            ptrs.add(e.cluster_device_ptr())
            for x, y in zip((LL, W, gp), again):
                assert same_bits(x, y)
        assert len(ptrs) == 2
    finally:
        e.close()
    RL, RW, Rgp = PR.mstep_window(off, cell, lgl, w, q, 1e-3, gk)
    assert same_bits(gp[:, :Vk], gk)
    assert np.abs(LL - RL).max() <= 1e-9
    assert (np.abs(W - RW) <= 1e-12 * np.maximum(np.abs(RW), 1.0)).all()
    cov = RW > 0
    fr, Rfr = gp[:, Vk:], Rgp[:, Vk:]
    ulp = np.abs(fr.view(np.int32).astype(np.int64) - Rfr.view(np.int32).astype(np.int64))
    assert ulp[cov].max(initial=0) <= 2
    assert same_bits(fr[~cov], np.broadcast_to(q[:, None, :], fr.shape)[~cov])
    assert (~cov[:, C - 1]).all()


def test_argument_errors(m):
    rng = np.random.default_rng(3)
    _, sp = make_sp(m, rng, 200, 4, 50, 0.2, 1.5)
    e = staged(m, sp, 7)
    try:
        DmxError = m["capi"].DmxError
        with pytest.raises(DmxError, match="run_singlet"):
            e.cluster_estep_known(2, 1, 3, np.zeros((2, 4)))
        e.run_singlet()
        with pytest.raises(DmxError, match="columns"):
            e.cluster_estep_known(2, 2, 3, np.zeros((2, 5)))          # 2 + 6 != 7
        with pytest.raises(DmxError, match="columns"):
            e.cluster_estep_known(7, 7, 0, np.zeros((7, 7)))          # M < 1
        with pytest.raises(DmxError, match="known columns"):
            e.cluster_set_known(np.zeros((200, 7, 3), dtype=np.float32))   # no free column left
        e.cluster_set_known(np.zeros((199, 1, 3), dtype=np.float32))
        with pytest.raises(DmxError, match="known rows have 199 SNPs"):
            e.cluster_mstep_window(np.zeros((50, 6)), 2, 3, np.zeros((200, 3), dtype=np.float32))
        e.cluster_set_known(np.zeros((200, 1, 3), dtype=np.float32))
        with pytest.raises(DmxError, match="no E-step weights"):
            e.cluster_mstep_window(None, 2, 3, np.zeros((200, 3), dtype=np.float32))
    finally:
        e.close()


def test_determinism_and_no_interference(m):
    """The new calls give the same bits twice and leave K1's and K2's results, the stage cache and the plain E-step's results alone."""
    rng = np.random.default_rng(29)
    S, B, Vk, R, M = 800, 300, 4, 3, 2
    V = Vk + R * M
    raw, sp = make_sp(m, rng, S, V, B, 0.2, 1.5)
    g = np.stack([m["engine"].geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    q = m["cluster"].hwe_prior(rng.integers(0, 20, S), rng.integers(0, 20, S))
    log_pi = np.log(rng.dirichlet(np.ones(Vk + M), size=R))
    e = staged(m, sp, V, g)
    try:
        e.run_singlet()
        e.run_doublet()
        sing, grid = e.get_singlet(), e.get_doublet()
        stage = e.get_cluster_stage()
        outs = []
        for _ in range(2):
            ll, cs = e.cluster_estep_known(R, Vk, M, log_pi)
            wk, wf = e.cluster_known_weights()
            e.cluster_set_known(g[:, :Vk])
            outs.append((ll, cs, wk, wf) + tuple(e.cluster_mstep_window(None, R, M, q)))
        for x, y in zip(*outs):
            assert same_bits(x, y)
        for x, y in zip(sing, e.get_singlet()):
            assert same_bits(x, y)
        for x, y in zip(grid, e.get_doublet()):
            assert same_bits(x, y)
        for x, y in zip(stage, e.get_cluster_stage()):
            assert same_bits(x, y)
    finally:
        e.close()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def read_best(path):
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        col = {n: i for i, n in enumerate(head)}
        return {t[col["BARCODE"]]: t[col["BEST"]] for t in (ln.rstrip("\n").split("\t") for ln in f)}


def partial_case(m, seed, V=8, B=4000, S=10000, delta=0.1, rbar=1.25, dense=False):
    rng = np.random.default_rng(seed)
    raw, sp = make_sp(m, rng, S, V, B, 1.0 if dense else delta, rbar, dense)
    g = m["engine"].geno_from_gt(raw.alleles, 0.01).reshape(S, V, 3)
    return sp, host_pileup(m, sp), g, [m["synth"].barcode_name(c) for c in range(B)]


def scores(m, sp, barcodes, prefix, known, dropped, n_unknown):
    """(the dropped donors' singlets called SNG- of their matched UNK, the known donors' singlets called SNG- of the right donor, the
    doublets called DBL-, the known x unknown doublets called DBL-, the UNK -> donor map)."""
    best = read_best(prefix + ".best")
    calls = [best.get(b, "") for b in barcodes]
    name = {f"donor{v}": v for v in known}
    kcall = np.array([name.get(c[4:], -1) if c.startswith("SNG-") else -1 for c in calls])
    ucall = np.array([int(c[len("SNG-UNK"):]) if c.startswith("SNG-UNK") else -1 for c in calls])
    is_dbl = np.array([c.startswith("DBL-") for c in calls])
    t0, t1 = sp.truth[:, 0], sp.truth[:, 1]
    singlet = t1 < 0
    didx = {v: i for i, v in enumerate(dropped)}
    truth_u = np.array([didx.get(int(t), -1) if s else -1 for t, s in zip(t0, singlet)])
    lab = m["cluster"].match_labels(truth_u, ucall, len(dropped), n_unknown)
    mapped = np.where(ucall >= 0, lab[np.maximum(ucall, 0)], -1)
    dsing = truth_u >= 0
    ksing = singlet & np.isin(t0, known)
    mixed = ~singlet & (np.isin(t0, dropped) != np.isin(t1, dropped))
    assert mixed.any()
    return (float((mapped[dsing] == truth_u[dsing]).mean()), float((kcall[ksing] == t0[ksing]).mean()), float(is_dbl[~singlet].mean()),
            float(is_dbl[mixed].mean()), lab)


def known_only_rate(m, pl, g, known, barcodes, sp, prefix):
    ids = [f"donor{v}" for v in known]
    m["engine"].demuxlet_run(pl, np.ascontiguousarray(g[:, known]), ids, (0.0, 0.5), prefix, barcodes=barcodes)
    best = read_best(prefix + ".best")
    calls = [best.get(b, "") for b in barcodes]
    k = np.array([known[ids.index(c[4:])] if c.startswith("SNG-") and c[4:] in ids else -1 for c in calls])
    ks = (sp.truth[:, 1] < 0) & np.isin(sp.truth[:, 0], known)
    return float((k[ks] == sp.truth[ks, 0]).mean())


# measured on an MI355X: every case recovers the dropped donors' singlets at 1.000, the known donors' singlets at
# the rate of demuxlet_run on the known columns alone (1.000) and 1.000 of the doublets, known x unknown ones included.  A dense layout with
# M = 2 is not here: every barcode covers the same SNPs, the random halves of the start are the same mixture, and all restarts keep
# both unknown donors in one column (limits).
@pytest.mark.parametrize("case", ["sparse M=2", "sparse M=1", "dense M=1", "M too large"])
def test_recovery(m, tmp_path, case):
    dense = case.startswith("dense")
    dropped = {"sparse M=2": [5, 7], "sparse M=1": [3], "dense M=1": [6], "M too large": [2]}[case]
    M = 2 if case == "M too large" else len(dropped)
    sp, pl, g, barcodes = partial_case(m, {"sparse M=2": 11, "sparse M=1": 12, "dense M=1": 13, "M too large": 14}[case],
                                       S=2000 if dense else 10000, dense=dense)
    if not dense:
        npc = np.diff(sp.cell_pair_off)
        assert 800 <= npc.mean() <= 1200 and 0.07 <= (sp.truth[:, 1] >= 0).mean() <= 0.13
    known = [v for v in range(8) if v not in dropped]
    pre = str(tmp_path / "o")
    res = m["partial"].partial_run(pl, np.ascontiguousarray(g[:, known]), [f"donor{v}" for v in known], M, pre, restarts=8, seed=5,
                                   barcodes=barcodes)
    base = known_only_rate(m, pl, g, known, barcodes, sp, str(tmp_path / "k"))
    s0 = scores(m, sp, barcodes, pre, known, dropped, M)
    s1 = scores(m, sp, barcodes, pre + ".r1", known, dropped, M)
    print(f"{case}: final pass unknown {s0[0]:.4f} known {s0[1]:.4f} (alone {base:.4f}) doublets {s0[2]:.4f} known x unknown {s0[3]:.4f}; "
          f"round 1 unknown {s1[0]:.4f} known {s1[1]:.4f} doublets {s1[2]:.4f}; iterations {res['iterations']} restart {res['restart']}; "
          f"UNK map {s0[4].tolist()}; calls per UNK {[sum(v == f'SNG-UNK{j}' for v in read_best(pre + '.best').values()) for j in range(M)]}")
    for s in (s0, s1):
        assert s[0] >= 0.99
        assert s[1] >= base - 0.005
        assert s[2] >= 0.95 and s[3] >= 0.95
    assert res["sample_ids"] == [f"donor{v}" for v in known] + [f"UNK{j}" for j in range(M)]
    assert same_bits(res["gp"][:, :len(known)], g[:, known])
    em = (tmp_path / "o.em.tsv").read_text().splitlines()
    assert em[0] == "ITER\tRESTART\tLLK\tPI" and len(em) == 1 + 8 * res["iterations"]
    assert all(len(r.split("\t")[3].split(",")) == len(known) + M for r in em[1:])
    clust = (tmp_path / "o.clust.tsv").read_text().splitlines()
    assert {ln.split("\t")[4] for ln in clust[1:]} <= {f"UNK{j}" for j in range(M)}


def test_determinism_and_match(m, tmp_path):
    sp, pl, g, barcodes = partial_case(m, 21, V=5, B=1500, S=4000)
    known = [0, 1, 2, 3]
    ids = [f"donor{v}" for v in known]
    outs = []
    for run in ("a", "b"):
        m["partial"].partial_run(pl, np.ascontiguousarray(g[:, known]), ids, 2, str(tmp_path / run), restarts=3, seed=7, barcodes=barcodes,
                                 match=True)
        outs.append(sorted(p.name[1:] for p in tmp_path.iterdir() if p.name.startswith(run + ".")))
    assert outs[0] == outs[1] and ".match.tsv" in outs[0] and ".r1.best" in outs[0]
    for ext in outs[0]:
        assert (tmp_path / ("a" + ext)).read_bytes() == (tmp_path / ("b" + ext)).read_bytes(), ext
    rows = [ln.split("\t") for ln in (tmp_path / "a.match.tsv").read_text().splitlines()[1:]]
    assert {r[0] for r in rows} == {"UNK0", "UNK1"} and {r[1] for r in rows} == set(ids)


# measured on an MI355X: 1.3 s for the whole run (29 EM iterations, the final pass, one round), every singlet and doublet right; the
# budget leaves a factor of ten
def test_full_size_cfg6_shape(m, tmp_path):
    """20 000 barcodes x 100 000 SNPs, ~2 000 covered SNPs per barcode (cfg6's shape), 16 donors of which 12 are known, M = 4, R = 8."""
    torch = m["torch"]
    from demuxlet_amd import synth_torch
    V, B, S, M = 16, 20_000, 100_000, 4
    rng = np.random.default_rng(0xC6)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    dev = torch.device("cuda", 0)
    dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
    dp = synth_torch.make_device_pileup(dosage, B, 0.02, 1.25, seed=0xC6C6, device=dev)
    h = dp.host_slice(0, B)
    truth = dp.truth.cpu().numpy()
    z = np.zeros(B, dtype=np.int32)
    pl = m["engine"].HostPileup(rd_totl=z, rd_pass=z, rd_uniq=z, **h)
    del dp, dosage
    torch.cuda.empty_cache()
    g = m["engine"].geno_from_gt(raw.alleles, 0.01).reshape(S, V, 3)
    barcodes = [m["synth"].barcode_name(c) for c in range(B)]
    dropped = [3, 8, 12, 15]
    known = [v for v in range(V) if v not in dropped]
    t0 = time.perf_counter()
    res = m["partial"].partial_run(pl, np.ascontiguousarray(g[:, known]), [f"donor{v}" for v in known], M, str(tmp_path / "f"), restarts=8,
                                   seed=1, barcodes=barcodes)
    wall = time.perf_counter() - t0

    class T:
        pass
    sp = T()
    sp.truth = truth
    s = scores(m, sp, barcodes, str(tmp_path / "f"), known, dropped, M)
    print(f"cfg6 shape 12 known + 4 unknown: wall {wall:.1f} s, iterations {res['iterations']}, unknown {s[0]:.4f} known {s[1]:.4f} "
          f"doublets {s[2]:.4f} known x unknown {s[3]:.4f}")
    assert s[0] >= 0.99 and s[1] >= 0.99 and s[2] >= 0.95
    assert wall < 15.0


def test_cli_on_pileup_dump(m, tmp_path):
    sp, pl, g, barcodes = partial_case(m, 31, V=4, B=600, S=3000)
    d = m["refine"].PileupDump([f"donor{v}" for v in range(3)], [(1, 100 + s, "A", "G") for s in range(sp.n_snps)],
                               np.ascontiguousarray(g[:, :3]), barcodes, pl)
    p = tmp_path / "x.pileup.txt"
    m["refine"].write_pileup_txt(str(p), d)
    assert m["partial"].main(["--pileup", str(p), "--n-unknown", "1", "--out", str(tmp_path / "c"), "--restarts", "2", "--match"]) == 0
    for ext in (".best", ".single", ".sing2", ".r1.best", ".em.tsv", ".clust.tsv", ".match.tsv"):
        assert (tmp_path / ("c" + ext)).stat().st_size > 0, ext
    s = scores(m, sp, barcodes, str(tmp_path / "c"), [0, 1, 2], [3], 1)
    assert s[0] >= 0.95 and s[1] >= 0.95
    rid = {ln.split("\t")[1] for ln in (tmp_path / "c.clust.tsv").read_text().splitlines()[1:]}
    assert rid and rid <= {str(100 + i) for i in range(sp.n_snps)}
