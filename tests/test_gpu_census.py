"""GPU (-m gpu): donor shares of a read pool (Engine.census_step / Engine.census, census.census_run, ambient="census").

One pass is checked against the float64 numpy restatement of tests/census_ref.py with tolerances computed from the case's own counts:
  |d acc_v| <= 2^-52 (T + V + 8) acc_v, T = reads + 2 pairs (the terms the sum is made of: all non-negative, no log on that path);
  |d ll|    <= 2^-52 (N + 3) sum|log P_r| + 1.12 2^-52 sum|log P_r| (N terms, and dmx_log's bound of DESIGN.md section 4);
  counts equal.
Then layouts and read-count widths, edge cases, bit reproducibility, the driver against the restatement's, recovery of known shares,
the census as the soup profile of ambient.py, the argument errors and the command line end to end."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import census_ref as R

pytestmark = pytest.mark.gpu
U = R.U
TRUE8 = np.array([.4, .25, .15, .1, .05, .03, .02, 0.0])


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import ambient, build, capi, census, engine, refine, synth
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    mat, err = engine.phred_tables()
    return dict(torch=torch, capi=capi, engine=engine, refine=refine, synth=synth, ambient=ambient, census=census, mat=mat, err=err)


def open_engine(m, g, pl):
    e = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    e.set_genotypes(g); e.set_pileup(pl)
    return e


def make_case(m, seed, B, S, V, n_reads, shares=None, **kw):
    rng = np.random.default_rng(seed)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = R.gt_rows(raw.alleles, 0.01)
    shares = rng.dirichlet(np.ones(V)) if shares is None else shares
    pl = R.make_pool(rng, raw.alleles, shares, B, n_reads, **kw)
    return rng, g, pl


def bounds(ref, V):
    T = ref.n_read + 2 * ref.n_pair
    return U * (T + V + 8) * ref.acc, U * (ref.n_read + 3) * ref.abs_log + 1.12 * U * ref.abs_log


def check_group(m, got, k, fl, d, valid, group, w, label=""):
    """Group k of a census_step result against the restatement."""
    acc, ll, gap, n_read, n_pair = got
    V = d.shape[1]
    ref = R.step(fl, d, valid, np.asarray(group) == k, w, m["mat"], m["err"])
    assert n_read[k] == ref.n_read and n_pair[k] == ref.n_pair, (label, k)
    tol_acc, tol_ll = bounds(ref, V)
    da, dl = np.abs(acc[k] - ref.acc), abs(ll[k] - ref.ll)
    print(f"{label} group {k}: N {ref.n_read} pairs {ref.n_pair} max d acc / bound {np.max(da / np.maximum(tol_acc, 1e-300)):.3f} "
          f"d ll / bound {dl / max(tol_ll, 1e-300):.3f}")
    assert np.all(da <= tol_acc), (label, k, float(np.max(da / np.maximum(tol_acc, 1e-300))))
    assert dl <= tol_ll, (label, k, dl, tol_ll)
    if ref.n_read:
        assert abs(gap[k] - ref.gap) <= tol_acc.max() + 8 * U * ref.n_read        # gap = N (max acc / N - 1): the largest acc's error and a few roundings of N
    else:
        assert gap[k] == 0.0 and ll[k] == 0.0 and not acc[k].any()
    return ref


def share_kinds(rng, V, G):
    out = {"uniform": np.full((G, V), 1.0 / V), "dirichlet": rng.dirichlet(np.ones(V), size=G)}
    if V >= 2:
        z = rng.dirichlet(np.ones(V), size=G)
        z[:, rng.choice(V, max(1, V // 3), replace=False)] = 0.0
        z[:, 0] += 1e-3                                  # (never an all-zero row)
        out["zeros"] = z / z.sum(axis=1, keepdims=True)
    return out


@pytest.mark.parametrize("B,S,V,n_reads,G", [
    (50, 500, 1, 4000, 1),
    (120, 1500, 3, 15000, 2),
    (300, 4000, 33, 30000, 3),
    (100, 800, 64, 12000, 1),
    (80, 700, 65, 12000, 2),
    (60, 600, 130, 10000, 1),
])
def test_step_against_the_restatement(m, B, S, V, n_reads, G):
    rng, g, pl = make_case(m, 100 * V + G, B, S, V, n_reads)
    fl = R.flatten(pl)
    d, valid = R.dosage(g)
    group = rng.integers(0, G, B).astype(np.int32)
    group[rng.random(B) < 0.1] = -1
    e = open_engine(m, g, pl)
    try:
        for kind, w in share_kinds(rng, V, G).items():
            assert np.all(np.abs(w.sum(axis=1) - 1.0) <= 1e-12)
            got = e.census_step(group, w, n_groups=G)
            for k in range(G):
                check_group(m, got, k, fl, d, valid, group, w[k], f"V={V} {kind}")
        info = e.census_info()
    finally:
        e.close()
    assert info["n_steps"] == 1 and info["n_invalid_snps"] == 0 and info["n_groups"] == G and info["n_samples"] == V
    assert info["dosage_bytes"] == S * V * 8 and info["n_chunks"] >= G and info["partial_bytes"] == info["n_chunks"] * (V + 1) * 8


def test_layouts_and_widths(m):
    rng, g, pl = make_case(m, 7, 40, 300, 5, 6000)
    fl = R.flatten(pl)
    d, valid = R.dosage(g)
    group = (np.arange(40) % 2).astype(np.int32)
    w = rng.dirichlet(np.ones(5), size=2)
    res = {}
    for name, p in (("sparse", pl), ("dense", R.to_dense(pl))):
        for width in (1, 2, 4):
            q = m["engine"].HostPileup(p.n_cells, p.n_snps, p.cell_pair_off, p.cell_read_off, p.pair_snp,
                                       np.asarray(p.pair_nrd).astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[width]), p.reads, p.rd_totl,
                                       p.rd_pass, p.rd_uniq)
            e = open_engine(m, g, q)
            try:
                res[name, width] = e.census_step(group, w)
            finally:
                e.close()
    assert R.to_dense(pl).pair_snp is None and (np.asarray(R.to_dense(pl).pair_nrd) == 0).any()
    for name in ("sparse", "dense"):
        for k in range(2):
            check_group(m, res[name, 1], k, fl, d, valid, group, w[k], name)
        for width in (2, 4):
            for x, y in zip(res[name, 1], res[name, width]):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (name, width)


def edge_case(m):
    """Barcode 0: 230 pairs of one read (four tiles), SNP 7 among them; barcode 1: a pair of 9 and a pair of 300 reads; barcode 2: a pair
    without stored reads and a normal one; barcode 3: reads of quality 0 and 93; barcode 4: one read; barcodes 5-9: a few reads each.
    SNP 7 has an all-zero row for donor 2."""
    rng = np.random.default_rng(11)
    S, V, B = 260, 4, 10
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = R.gt_rows(raw.alleles, 0.01)
    g[7, 2] = 0.0
    cell, snp, byte = [], [], []

    def add(c, s, al, bq):
        cell.append(c); snp.append(s); byte.append((al << 7) | bq)
    for s in range(230):
        add(0, s, int(rng.integers(0, 2)), int(rng.integers(10, 41)))
    for _ in range(9):
        add(1, 20, int(rng.integers(0, 2)), int(rng.integers(10, 41)))
    for _ in range(300):
        add(1, 100, int(rng.random() < 0.4), int(rng.integers(10, 41)))
    add(2, 31, 1, 30)
    for bq in (0, 93, 0, 93):
        add(3, 40 + bq, int(rng.integers(0, 2)), bq)
        add(3, 41 + bq, 1, bq)
    add(4, 55, 0, 37)
    for c in range(5, 10):
        for s in rng.choice(S, 6, replace=False):
            add(c, int(s), int(rng.integers(0, 2)), int(rng.integers(10, 41)))
    pl = R.build_pileup(B, S, cell, snp, byte, nrd_dtype=np.uint16, extra_pairs=[(2, 30)])
    return rng, g, pl


def test_edges(m):
    rng, g, pl = edge_case(m)
    fl = R.flatten(pl)
    assert (fl.nrd == 0).sum() == 1 and set([9, 300]) <= set(fl.nrd.tolist()) and np.diff(pl.cell_pair_off)[0] == 230
    d, valid = R.dosage(g)
    assert (~valid).sum() == 1 and not valid[7]
    V, G = 4, 70
    group = np.array([0, 1, 2, 3, 4, 6, 6, 69, 69, -1], dtype=np.int32)        # group 5 and 7..68 have no barcode; group 4 is one read
    w = rng.dirichlet(np.ones(V), size=G)
    e = open_engine(m, g, pl)
    try:
        got = e.census_step(group, w)
        assert got[0].shape == (G, V)
        for k in range(G):
            ref = check_group(m, got, k, fl, d, valid, group, w[k], "edges")
        assert got[3][4] == 1 and got[4][4] == 1 and got[3][5] == 0                  # the group of one read; an empty group
        assert got[3][0] == 229 and got[4][0] == 229                                 # barcode 0 without the pair at the invalid SNP
        assert got[4][2] == 1                                                        # barcode 2: the pair without stored reads is not counted
        assert e.census_info()["n_invalid_snps"] == 1
        one = e.census_step(np.where(group >= 0, 0, -1).astype(np.int32), w[:1])     # G = 1
        check_group(m, one, 0, fl, d, valid, np.where(group >= 0, 0, -1), w[0], "edges G=1")
        none = e.census_step(np.full(10, -1, dtype=np.int32), w[:3], n_groups=3)      # every barcode unused
        assert not none[0].any() and not none[1].any() and not none[2].any() and not none[3].any() and not none[4].any()
        r = e.census(np.full(10, -1, dtype=np.int32), n_groups=2, w0=w[:2])
        assert np.array_equal(r["w"], w[:2]) and not r["ll"].any() and r["converged"].tolist() == [1, 1] and not r["n_read"].any()
    finally:
        e.close()
    del ref


def same_bits(x, y):
    return all(np.array_equal(np.atleast_1d(u).view(np.uint8), np.atleast_1d(v).view(np.uint8)) for u, v in zip(x, y))


def test_bits(m):
    torch = m["torch"]
    rng, g, pl = make_case(m, 13, 200, 1200, 12, 25000)
    V, G, B = 12, 5, 200
    group = rng.integers(-1, G, B).astype(np.int32)
    w = rng.dirichlet(np.ones(V), size=G)
    a = rng.uniform(0.05, 0.95, size=1200)
    assign = rng.integers(0, V, B).astype(np.int32)
    grid = np.array([0.0, 0.1, 0.3])

    def others(e):
        llks, llk0s = e.get_singlet()
        grid_, l00, summ = e.get_doublet()
        return [llks, llk0s, grid_, l00, summ.view(np.uint8)]

    e = open_engine(m, g, pl)
    try:
        r1 = e.census_step(group, w)
        r2 = e.census_step(group, w)
        assert same_bits(r1, r2)
        d_group = torch.from_numpy(group).to("cuda:0")
        assert same_bits(r1, e.census_step(int(d_group.data_ptr()), w, n_groups=G))
        for k in range(G):
            alone = e.census_step(np.where(group == k, 0, -1).astype(np.int32), w[k:k + 1])
            assert same_bits([x[k] for x in r1], [x[0] for x in alone]), k
        c1 = e.census(group, n_groups=G)
        e.run(); e.sync()
        base = others(e)
        amb = e.ambient_profile(assign, a, grid)
        assert same_bits(r1, e.census_step(group, w))
        c2 = e.census(group, n_groups=G)
        assert same_bits([c1[n] for n in sorted(c1)], [c2[n] for n in sorted(c2)])
        assert same_bits(base, others(e))
        ll = np.zeros_like(amb[0]); ns = np.zeros_like(amb[1]); nr = np.zeros_like(amb[2])
        m["capi"].check(e._L.dmx_engine_get_ambient(e._h, ll.ctypes.data, ns.ctypes.data, nr.ctypes.data))
        assert same_bits(amb, (ll, ns, nr))
    finally:
        e.close()
    # a fresh engine that ran nothing else gives the census the same bits
    e = open_engine(m, g, pl)
    try:
        c3 = e.census(group, n_groups=G)
    finally:
        e.close()
    assert same_bits([c1[n] for n in sorted(c1)], [c3[n] for n in sorted(c3)])


@pytest.fixture(scope="module")
def driver_case(m):
    """Three groups of very different sizes (they stop after different numbers of passes) and the restatement's SQUAREM run of each."""
    rng, g, pl = make_case(m, 17, 90, 1500, 8, 14000, shares=TRUE8, cell_shares=np.r_[np.full(60, 0.9 / 60), np.full(30, 0.1 / 30)])
    group = np.r_[np.zeros(60), np.ones(25), np.full(5, 2)].astype(np.int32)
    fl = R.flatten(pl)
    d, valid = R.dosage(g)
    ref = [R.run(fl, d, valid, group == k, m["mat"], m["err"]) for k in range(3)]
    return g, pl, group, fl, d, valid, ref


def test_driver(m, driver_case):
    g, pl, group, fl, d, valid, ref = driver_case
    V, G, tol = 8, 3, 1e-4
    e = open_engine(m, g, pl)
    try:
        r = e.census(group, n_groups=G)
        info = e.census_info()
        plain = e.census(group, n_groups=G, accelerate=False, max_steps=50000)         # (plain EM needs thousands of passes)
        short = e.census(group, n_groups=G, max_steps=3)
        alone = [e.census(np.where(group == k, 0, -1).astype(np.int32), n_groups=1) for k in range(G)]
    finally:
        e.close()
    print("steps", r["n_steps"], "plain", plain["n_steps"], "restatement", [x["n_steps"] for x in ref])
    assert r["converged"].tolist() == [1, 1, 1] and info["n_steps"] == r["n_steps"].max()
    assert len(set(r["n_steps"].tolist())) > 1                                       # the groups stopped at different passes
    for k in range(G):
        assert abs(r["w"][k].sum() - 1.0) <= 1e-12 and (r["w"][k] >= 0).all()
        s = R.step(fl, d, valid, group == k, r["w"][k], m["mat"], m["err"])
        tol_acc, tol_ll = bounds(s, V)
        assert s.gap <= tol + U * (s.n_read + 2 * s.n_pair + V + 8) * s.n_read, (k, s.gap)
        assert abs(r["ll"][k] - ref[k]["ll"]) <= tol + tol_ll, (k, r["ll"][k], ref[k]["ll"])
        assert r["gap"][k] <= tol and r["n_read"][k] == s.n_read == ref[k]["n_read"] and r["n_pair"][k] == s.n_pair
        assert abs(r["ll"][k] - s.ll) <= tol_ll
        # a stopped group is frozen: while the others go on it keeps the bits it has when run alone
        assert same_bits([r[n][k] for n in sorted(r)], [alone[k][n][0] for n in sorted(r)]), k
        assert plain["converged"][k] == 1 and plain["gap"][k] <= tol
        assert abs(plain["ll"][k] - r["ll"][k]) <= 2 * tol + tol_ll
    assert plain["n_steps"].max() > r["n_steps"].max()
    for k in range(G):
        if r["n_steps"][k] > 3:
            assert short["n_steps"][k] == 3 and short["converged"][k] == 0 and short["gap"][k] > tol
        else:
            assert short["n_steps"][k] == r["n_steps"][k] and short["converged"][k] == 1
    assert (short["n_steps"] == 3).any()


def test_recovery(m):
    """8 donors with shares .4 .25 .15 .1 .05 .03 .02 0, 4 000 SNPs, 40 000 reads drawn, GT rows with error 0.01, base qualities 10-40.
    tests/test_census_cpu.py runs the restatement on this seed: its error is 0.014 (< 0.02), so the threshold is the issue's 0.03."""
    rng = np.random.default_rng(2201)
    raw = m["synth"].make_raw_genotypes(rng, 4000, 8)
    g = R.gt_rows(raw.alleles, 0.01)
    pl = R.make_pool(rng, raw.alleles, TRUE8, 300, 40000)
    e = open_engine(m, g, pl)
    try:
        r = e.census(np.zeros(300, dtype=np.int32))
    finally:
        e.close()
    err = float(np.abs(r["w"][0] - TRUE8).max())
    print(f"recovery: max |w - truth| = {err:.4f}, absent donor {r['w'][0, 7]:.5f}, steps {int(r['n_steps'][0])}")
    assert r["converged"][0] == 1 and err <= 0.03 and r["w"][0, 7] < 0.01


def test_ambient_census(m, tmp_path):
    """ambient="census" on synth.make_ambient_pileup: the per-barcode estimates stay within the asserts of test_gpu_ambient.py's
    per-barcode recovery test; ambient="reads" writes the bytes it writes when handed ambient_from_reads' array."""
    A, synth = m["ambient"], m["synth"]
    levels = np.array([0.0, 0.05, 0.1, 0.2, 0.3])
    B, S, V = 600, 20000, 8
    rng = np.random.default_rng(41)
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([m["engine"].geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    sp, rho, a_true = synth.make_ambient_pileup(rng, raw.alleles, B, 0.1, 1.25, levels[np.arange(B) % len(levels)])
    pl = m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads, sp.rd_totl,
                                sp.rd_pass, sp.rd_uniq)
    grid = A.default_grid()
    assign = sp.truth[:, 0].copy()
    e = open_engine(m, g, pl)
    try:
        a = A.ambient_from_census(e, g)
        a_reads = A.ambient_from_reads(e, g)
        ll, n_snp, _ = e.ambient_profile(assign, a, grid)
    finally:
        e.close()
    assert a.shape == (S,) and np.all((a >= 0) & (a <= 1))
    print(f"rms(a_census - a_true) = {np.sqrt(np.mean((a - a_true) ** 2)):.4f}, rms(a_reads - a_true) = {np.sqrt(np.mean((a_reads - a_true) ** 2)):.4f}")
    s = A.summarize(ll, grid)
    med_err = {float(r): float(np.median(np.abs(s.rho[rho == r] - r))) for r in levels}
    zero_lo = float((s.rho_lo[rho == 0.0] == 0.0).mean())
    covered = (s.rho_lo <= rho) & (rho <= s.rho_hi)
    print("median |rho^ - rho|", med_err, "rho0_lo_is_0", zero_lo, "covered", float(covered.mean()))
    assert 1500 < np.median(n_snp) < 2500
    for r in levels:
        assert med_err[float(r)] <= 0.05, (r, med_err)
    assert zero_lo >= 0.8, zero_lo
    assert covered.mean() >= 0.8, covered.mean()
    # "reads" keeps its bytes; "census" runs through ambient_run
    small = np.arange(B) < 40
    keep = np.repeat(small, np.diff(sp.cell_pair_off))
    po = np.concatenate([[0], np.cumsum(np.diff(sp.cell_pair_off)[small])]).astype(np.int64)
    ro = np.concatenate([[0], np.cumsum(np.diff(sp.cell_read_off)[small])]).astype(np.int64)
    pl2 = m["engine"].HostPileup(40, S, po, ro, np.asarray(sp.pair_snp)[keep], np.asarray(sp.pair_nrd)[keep], np.asarray(sp.reads)[:ro[-1]],
                                 sp.rd_totl[:40], sp.rd_pass[:40], sp.rd_uniq[:40])
    samples = [f"S{j}" for j in range(V)]
    bcs = [synth.barcode_name(c) for c in range(40)]
    r0 = A.ambient_run(pl2, g, samples, str(tmp_path / "r0"), ambient="reads", barcodes=bcs)
    A.ambient_run(pl2, g, samples, str(tmp_path / "r1"), best=str(tmp_path / "r0.best"), ambient=r0["ambient"], barcodes=bcs)
    for ext in (".ambient.tsv", ".ambient_pool.tsv"):
        assert (tmp_path / ("r0" + ext)).read_bytes() == (tmp_path / ("r1" + ext)).read_bytes()
    rc = A.ambient_run(pl2, g, samples, str(tmp_path / "rc"), best=str(tmp_path / "r0.best"), ambient="census", barcodes=bcs)
    assert rc["ambient"].shape == (S,) and (tmp_path / "rc.ambient.tsv").exists()


def test_argument_errors(m):
    capi = m["capi"]
    rng, g, pl = make_case(m, 19, 20, 100, 4, 800)
    V, B = 4, 20
    w = np.full((2, V), 0.25)
    grp = (np.arange(B) % 2).astype(np.int32)

    def raises(code, fn, *a, **k):
        with pytest.raises(capi.DmxError) as ei:
            fn(*a, **k)
        assert ei.value.code == code, ei.value

    e = m["engine"].Engine(V, (0.0, 0.5), 0.5)
    try:
        e.B = 3                                                             # an empty pileup is staged, but no genotype matrix yet
        z = np.zeros(3, dtype=np.int32)
        e.set_pileup(m["engine"].HostPileup(3, 0, np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32),
                                            np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), z, z.copy(), z.copy()))
        raises(-3, e.census_step, np.zeros(3, dtype=np.int32), w[:1])
        raises(-3, e.census, np.zeros(3, dtype=np.int32))
    finally:
        e.close()
    e = m["engine"].Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g)
        e.B = B
        raises(-3, e.census_step, grp, w)                                   # genotypes, but no pileup yet
        raises(-3, e.census, grp)
        raises(-3, e.census_info)
        e.set_pileup(pl)
        with pytest.raises(capi.DmxError) as ei:
            capi.check(e._L.dmx_engine_get_census(e._h, None, None, None, None, None, None, None))
        assert ei.value.code == -3                                          # nothing computed yet
        raises(-1, e.census_step, grp, np.full((1025, V), 0.25), n_groups=1025)
        raises(-1, e.census, grp, n_groups=0)
        raises(-1, e.census_step, np.full(B, 2, dtype=np.int32), w, n_groups=2)          # group[b] = G
        raises(-1, e.census_step, np.full(B, -2, dtype=np.int32), w, n_groups=2)
        for bad in (np.array([[0.5, 0.5, 0.5, -0.5]] * 2), np.full((2, V), 0.26), np.array([[np.nan, 1, 0, 0]] * 2),
                    np.array([[1.0, 0, 0, 0], [0.25, 0.25, 0.25, 0.25 + 1e-9]])):
            raises(-1, e.census_step, grp, bad)
            raises(-1, e.census, grp, w0=bad)
        rq = capi.CensusStepRequest(B + 1, capi.DMX_MEM_HOST, grp.ctypes.data, 2, V, w.ctypes.data)
        assert e._L.dmx_engine_census_step(e._h, C.byref(rq)) == -1                  # n_cells does not match
        rq = capi.CensusStepRequest(B, capi.DMX_MEM_HOST, grp.ctypes.data, 2, V + 1, w.ctypes.data)
        assert e._L.dmx_engine_census_step(e._h, C.byref(rq)) == -1                  # n_samples does not match
        rq = capi.CensusStepRequest(B, 7, grp.ctypes.data, 2, V, w.ctypes.data)
        assert e._L.dmx_engine_census_step(e._h, C.byref(rq)) == -1                  # group_memory
        rq = capi.CensusStepRequest(B, capi.DMX_MEM_HOST, grp.ctypes.data, 2, V, None)
        assert e._L.dmx_engine_census_step(e._h, C.byref(rq)) == -1                  # no w
        with pytest.raises(ValueError):
            e.census_step(np.zeros(B + 1, dtype=np.int32), w)
        with pytest.raises(ValueError):
            e.census_step(grp, np.full((2, V + 1), 0.2))
        got = e.census_step(grp, w)                                         # and the engine still works
        assert got[3].sum() == len(pl.reads)
    finally:
        e.close()


def test_census_run_end_to_end(m, tmp_path):
    """From a dump written by the `demuxlet` binary's --pileup-only on synthetic SAM / VCF data: the three files parse, each group's
    shares sum to 1 and the profile is in [0, 1]; then --max-reads and --groups."""
    import sam_vcf_synth as sv
    census = m["census"]
    cli = Path(census.__file__).resolve().parent / "demuxlet"
    contigs = [("1", 30000), ("2", 20000)]
    samples = ["smC", "smA", "smB", "smD"]
    rng = np.random.default_rng(23)
    recs = sv.make_vcf(rng, contigs, 120, samples, tmp_path / "v.vcf.gz")
    bcs = [f"BC{i:02d}-1" for i in range(25)]
    sv.make_reads(rng, contigs, recs, 4000, bcs, tmp_path / "r.sam", tmp_path / "r.bam")
    subprocess.run([str(cli), "--sam", str(tmp_path / "r.sam"), "--vcf", str(tmp_path / "v.vcf.gz"), "--field", "GT", "--out", str(tmp_path / "o"),
                    "--pileup-only"], check=True, stderr=subprocess.DEVNULL)
    dump = str(tmp_path / "o.pileup.txt")
    d = m["refine"].read_pileup_txt(dump)
    V, S = len(d.sample_ids), d.pileup.n_snps

    def parse(prefix, names):
        rows = [x.split("\t") for x in Path(prefix + ".census.tsv").read_text().splitlines()]
        assert rows[0] == census.CENSUS_HEADER.rstrip("\n").split("\t") and len(rows) == 1 + len(names) * V
        grows = [x.split("\t") for x in Path(prefix + ".census_groups.tsv").read_text().splitlines()]
        assert grows[0] == census.GROUPS_HEADER.rstrip("\n").split("\t") and [x[0] for x in grows[1:]] == names
        prows = [x.split("\t") for x in Path(prefix + ".census_profile.tsv").read_text().splitlines()]
        assert prows[0] == census.PROFILE_HEADER.rstrip("\n").split("\t") and len(prows) == 1 + len(names) * S
        for k, name in enumerate(names):
            sh = [float(x[2]) for x in rows[1:] if x[0] == name]
            assert [x[1] for x in rows[1:] if x[0] == name] == d.sample_ids and abs(sum(sh) - 1.0) < 1e-5 and min(sh) >= 0.0
            n_read = int(grows[1 + k][3])
            assert abs(sum(float(x[3]) for x in rows[1:] if x[0] == name) - n_read) < 0.01 * V + 1e-6 * n_read
            assert int(grows[1 + k][7]) == 1 and float(grows[1 + k][5]) <= 1e-4 and int(grows[1 + k][6]) >= 1
        vals = [x[2] for x in prows[1:]]
        assert all(v == "NA" or 0.0 <= float(v) <= 1.0 for v in vals) and any(v != "NA" for v in vals)
        return grows

    assert census.main(["--pileup", dump, "--out", str(tmp_path / "c")]) == 0
    gr = parse(str(tmp_path / "c"), ["POOL"])
    assert int(gr[1][1]) == d.pileup.n_cells and int(gr[1][3]) > 500
    cut = int(np.median(d.pileup.rd_uniq))
    assert census.main(["--pileup", dump, "--out", str(tmp_path / "e"), "--max-reads", str(cut), "--no-accel", "--max-steps", "50000"]) == 0
    gr = parse(str(tmp_path / "e"), ["EMPTY", "CELLS"])
    assert int(gr[1][1]) == int((d.pileup.rd_uniq <= cut).sum()) and int(gr[1][1]) + int(gr[2][1]) == d.pileup.n_cells
    (tmp_path / "g.tsv").write_text("".join(f"{b}\t{'odd' if i % 2 else 'even'}\n" for i, b in enumerate(d.barcodes[:-3])))
    assert census.main(["--pileup", dump, "--out", str(tmp_path / "g"), "--groups", str(tmp_path / "g.tsv"), "--tol", "1e-5"]) == 0
    gr = parse(str(tmp_path / "g"), ["even", "odd"])
    assert int(gr[1][1]) + int(gr[2][1]) == d.pileup.n_cells - 3
