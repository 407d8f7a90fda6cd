"""GPU (-m gpu): the model-drawn null pool (Engine.redraw / dmx_engine_redraw, redraw.redraw_run).

The contract is integer hashes and individually rounded float64 operations, so the device's read bytes, genotypes and counts must EQUAL
the serial restatement of tests/redraw_ref.py — over barcodes of exactly 0, 1, 63, 64, 65 and 129 pairs (k_fit's skeleton: lane = pair,
64 pair headers per trip), dense and sparse layouts, read counts of 1, 2 and 4 bytes, a pair of 300 reads, pairs without stored reads,
every kind of hypothesis, alpha, rho, gp row and base quality the contract distinguishes, both draw modes, hyp on the host and on the device.  Then
the structure of the view, the bit properties, adoption by a second engine, no interference, the law on the device with the CPU test's
pool and seeds, every argument and state error, and redraw_run end to end.  DMX_ERR_NOMEM is left out: the outputs are the size of the
staged read array, which already fits.  18 cases, 3 s together."""
import ctypes as C

import numpy as np
import pytest

import fit_ref as F
import redraw_ref as R
from contract_emul import PAIR_COUNTS

pytestmark = pytest.mark.gpu
BQS = np.array([0, 1, 2, 13, 40, 93, 127], dtype=np.uint8)
ALPHAS = (0.0, 0.13, 0.5, 1.0)
RHOS = (0.0, 0.3, 1.0)
COUNT_KEYS = ("n_cells", "n_used", "n_singlet", "n_doublet", "n_pairs_drawn", "n_pairs_skipped", "n_reads_drawn", "n_reads_kept")


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import build, capi, engine, fit, redraw, refine, synth
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    mat, err = engine.phred_tables()
    return dict(torch=torch, capi=capi, engine=engine, refine=refine, synth=synth, fit=fit, redraw=redraw, mat=mat, err=err)


def host_pileup(m, sp, width=None, sparse=False):
    nrd = np.asarray(sp.pair_nrd)
    if width is not None:
        nrd = nrd.astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[width])
    snp = sp.pair_snp
    if snp is None and sparse:
        snp = np.tile(np.arange(sp.n_snps, dtype=np.int32), sp.n_cells)
    return m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, snp, nrd, sp.reads, sp.rd_totl, sp.rd_pass, sp.rd_uniq)


def staged(m, g, pl):
    e = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    e.set_genotypes(g); e.set_pileup(pl)
    return e


def edge_matrix(rng, S, V):
    """Soft rows, with the rows that matter: all zero, hard zeros in every position, a negative entry, a non-finite entry, subnormals."""
    g = rng.dirichlet(np.ones(3), size=(S, V)).astype(np.float32)
    sub = np.float32(1e-45)
    special = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0.5, 0.5, 0), (0, 0.25, 0.75), (0.5, 0, 0.5), (0.3, -0.1, 0.8), (np.nan, 0.5, 0.5),
               (sub, sub, sub), (sub, 0, sub), (0, sub, 0), (np.inf, 0, 0), (2.0, 3.0, 5.0)]
    for k, row in enumerate(special * 3):
        g[(7 * k + 3) % S, k % V] = np.array(row, dtype=np.float32)
    return g


def edge_pool(m, rng, counts, S, dense=False, deep=True):
    """Barcodes of exactly `counts` pairs (dense: S each) with 0 to 5 reads per pair at the listed base qualities; deep: one pair of 300
    reads in the second trip of the first barcode that has one."""
    cells = []
    for n in counts:
        snps = np.arange(S) if dense else np.sort(rng.choice(S, n, replace=False))
        nr = rng.choice([0, 1, 1, 1, 2, 3, 5], size=len(snps))
        cells.append([snps, nr])
    if deep:
        k = next(i for i, (s, _) in enumerate(cells) if len(s) > 64)
        cells[k][1][64] = 300
    nrd = np.concatenate([c[1] for c in cells]) if cells else np.zeros(0, dtype=np.int64)
    R_ = int(nrd.sum())
    reads = ((rng.integers(0, 2, size=R_) << 7) | BQS[rng.integers(0, len(BQS), size=R_)]).astype(np.uint8)
    po = np.concatenate([[0], np.cumsum([len(c[0]) for c in cells])]).astype(np.int64)
    ro = np.concatenate([[0], np.cumsum([int(c[1].sum()) for c in cells])]).astype(np.int64)
    t = np.ones(len(cells), dtype=np.int32)
    snp = None if dense else np.concatenate([c[0] for c in cells]).astype(np.int32)
    return m["synth"].SynthPileup(len(cells), S, po, ro, snp, nrd.astype(np.uint16 if deep else np.uint8), reads, t, t.copy(), t.copy(),
                                  np.full((len(cells), 2), -1, dtype=np.int32))


def edge_hypotheses(rng, B, V):
    """Unused, singlet and doublet in turn (every barcode count class gets each, the list being twice PAIR_COUNTS and more)."""
    hyp = np.full((B, 2), -1, dtype=np.int32)
    for b in range(B):
        kind = (b + b // 6) % 3
        if kind >= 1:
            hyp[b, 0] = rng.integers(0, V)
        if kind == 2 and V > 1:
            hyp[b, 1] = (hyp[b, 0] + 1 + rng.integers(0, V - 1)) % V
    hyp[B - 1] = (-1, 0)                                                         # v1 = -1: unused whatever v2 says
    alpha = np.array([ALPHAS[b % 4] for b in range(B)])
    return hyp, alpha


def run_redraw(m, g, pl, hyp, alpha, rho, a, device_hyp=False, **kw):
    e = staged(m, g, pl)
    try:
        h = hyp
        if device_hyp:
            d_hyp = m["torch"].from_numpy(np.ascontiguousarray(hyp, dtype=np.int32)).cuda()
            h = int(d_hyp.data_ptr())
        info = e.redraw(h, alpha, rho, a, **kw)
        out = e.get_redrawn()
        st = e.redrawn_pileup()
        assert st.n_cells == pl.n_cells and st.n_pairs == len(pl.pair_nrd) and st.n_reads == len(pl.reads)
        assert st.nrd_width == pl.pair_nrd.dtype.itemsize and bool(st.pair_snp) == (pl.pair_snp is not None) and not st.rd_totl
    finally:
        e.close()
    return out, info


def check(m, sp, g, hyp, alpha, rho, a, mode, width=None, sparse=False, device_hyp=False, seed=11, geno_seed=12, index_base=0):
    pl = host_pileup(m, sp, width, sparse)
    out, info = run_redraw(m, g, pl, hyp, alpha, rho, a, device_hyp, seed=seed, geno_seed=geno_seed, genotype_draw=mode, index_base=index_base)
    ref = R.redraw(pl, hyp, alpha, rho, a, g, m["mat"], m["err"], seed, geno_seed, R.DONOR if mode == "donor" else R.PAIR, index_base)
    assert np.array_equal(out["reads"], ref["reads"]), int((out["reads"] != ref["reads"]).sum())
    assert np.array_equal(out["geno"], ref["geno"])
    for k in COUNT_KEYS:
        assert info[k] == ref[k], (k, info[k], ref[k])
    assert info["genotype_draw"] == (1 if mode == "donor" else 0) and info["bytes_written"] >= info["n_reads_drawn"] and info["kernel_ms"] >= 0.0
    # structure: base qualities kept; only drawn pairs' bytes may change
    assert np.array_equal(out["reads"] & 127, pl.reads & 127)
    cell, snp, nrd, start, _ = F.host_pairs(pl.cell_pair_off, pl.pair_snp, pl.pair_nrd)
    same = np.ones(len(pl.reads), dtype=bool)
    for p in np.flatnonzero(out["geno"][:, 0] >= 0):
        same[start[p]:start[p] + nrd[p]] = False
    assert np.array_equal(out["reads"][same], pl.reads[same])
    assert not (out["geno"][np.asarray(hyp)[cell, 0] < 0] >= 0).any() and not (out["geno"][nrd == 0] >= 0).any()
    return out, info, ref


def soup(rng, B, S, kind):
    if kind is None:
        return None, None
    rho = np.full(B, kind) if kind in (0.0,) else np.array([RHOS[b % 3] for b in range(B)])
    a = rng.uniform(0.0, 1.0, size=S)
    a[:4] = (0.0, 1.0, 0.5, 0.0)[:min(S, 4)]
    return rho, a


@pytest.mark.parametrize("mode,width,rho_kind,device_hyp", [
    ("pair", 2, "mixed", False),
    ("donor", 2, "mixed", True),
    ("pair", 4, None, True),
    ("donor", 4, 0.0, False),
    ("pair", 1, "mixed", False),                   # no pair of 300 reads: one-byte read counts
    ("donor", 1, None, False),
])
def test_redraw_equals_the_restatement_sparse(m, mode, width, rho_kind, device_hyp):
    rng = np.random.default_rng(100 + width + (mode == "donor"))
    S, V = 140, 5
    counts = list(PAIR_COUNTS) * 2 + [int(x) for x in rng.integers(0, S + 1, size=6)]
    sp = edge_pool(m, rng, counts, S, deep=width > 1)
    g = edge_matrix(rng, S, V)
    hyp, alpha = edge_hypotheses(rng, sp.n_cells, V)
    rho, a = soup(rng, sp.n_cells, S, rho_kind)
    out, info, ref = check(m, sp, g, hyp, alpha, rho, a, mode, width, device_hyp=device_hyp)
    assert info["n_pairs_skipped"] > 0 and info["n_pairs_drawn"] > 300 and info["n_singlet"] > 3 and info["n_doublet"] > 3
    assert (sp.pair_nrd == 0).sum() > 20 and set((sp.reads & 127).tolist()) == set(BQS.tolist())
    if width > 1:
        assert sp.pair_nrd.max() == 300
    if rho_kind is not None:
        assert (out["reads"] != sp.reads).any()


@pytest.mark.parametrize("S,mode", [(1, "pair"), (63, "donor"), (64, "pair"), (65, "donor"), (129, "pair")])
def test_redraw_equals_the_restatement_dense_and_dense_equals_sparse(m, S, mode):
    rng = np.random.default_rng(200 + S)
    V, B = 4, 7
    sp = edge_pool(m, rng, [S] * B, S, dense=True, deep=S > 64)
    assert sp.pair_snp is None
    g = edge_matrix(rng, S, V) if S >= 63 else rng.dirichlet(np.ones(3), size=(S, V)).astype(np.float32)
    hyp, alpha = edge_hypotheses(rng, B, V)
    rho, a = soup(rng, B, S, "mixed")
    dense, _, _ = check(m, sp, g, hyp, alpha, rho, a, mode)
    sparse, _, _ = check(m, sp, g, hyp, alpha, rho, a, mode, sparse=True, width=4)
    assert dense["reads"].tobytes() == sparse["reads"].tobytes() and dense["geno"].tobytes() == sparse["geno"].tobytes()


@pytest.fixture(scope="module")
def pool(m):
    rng = np.random.default_rng(31)
    S, V, B = 400, 6, 90
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = np.stack([m["engine"].geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    g = (np.float32(0.8) * g + np.float32(0.2 / 3)).astype(np.float32)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.3, 1.6, doublet_rate=0.3, quals="edges")
    hyp = sp.truth.astype(np.int32).copy()
    hyp[::9] = (-1, -1)
    alpha = np.where(hyp[:, 1] >= 0, 0.5, 0.0)
    rho = rng.choice([0.0, 0.2], size=B); a = rng.uniform(0, 1, size=S)
    return sp, g, host_pileup(m, sp), hyp, alpha, rho, a


def test_bits_repeat_seed_and_index_base(m, pool):
    sp, g, pl, hyp, alpha, rho, a = pool
    e = staged(m, g, pl)
    one = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    try:
        e.redraw(hyp, alpha, rho, a, seed=5, geno_seed=6, genotype_draw="pair")
        r1 = e.get_redrawn()
        e.fit_profile(hyp, alpha, rho, a, 4)                                     # (something else in between)
        e.redraw(hyp, alpha, rho, a, seed=5, geno_seed=6, genotype_draw="pair")
        r2 = e.get_redrawn()
        assert r1["reads"].tobytes() == r2["reads"].tobytes() and r1["geno"].tobytes() == r2["geno"].tobytes()
        e.redraw(hyp, alpha, rho, a, seed=6, geno_seed=6, genotype_draw="pair")
        r3 = e.get_redrawn()
        assert (r3["reads"] != r1["reads"]).sum() > 100 and (r3["geno"] != r1["geno"]).any()
        e.redraw(hyp, alpha, rho, a, seed=5, geno_seed=7, genotype_draw="pair")  # PAIR mode does not look at geno_seed
        assert e.get_redrawn()["reads"].tobytes() == r1["reads"].tobytes()
        # barcode b of the pool = barcode 0 of the one-barcode pool hashed as index_base = b (here the pool itself sits at base 1000)
        e.redraw(hyp, alpha, rho, a, seed=5, geno_seed=6, genotype_draw="pair", index_base=1000)
        big = e.get_redrawn()
        one.set_genotypes(g)
        for b in (1, 2, 40, 89):
            assert hyp[b, 0] >= 0
            p0, p1, r0, r1_ = (int(x) for x in (pl.cell_pair_off[b], pl.cell_pair_off[b + 1], pl.cell_read_off[b], pl.cell_read_off[b + 1]))
            t = np.ones(1, dtype=np.int32)
            solo = m["engine"].HostPileup(1, pl.n_snps, np.array([0, p1 - p0], dtype=np.int64), np.array([0, r1_ - r0], dtype=np.int64),
                                          pl.pair_snp[p0:p1].copy(), pl.pair_nrd[p0:p1].astype(np.uint32), pl.reads[r0:r1_].copy(), t, t, t)
            one.set_pileup(solo)
            one.redraw(hyp[b:b + 1], alpha[b:b + 1], rho[b:b + 1], a, seed=5, geno_seed=6, genotype_draw="pair", index_base=1000 + b)
            got = one.get_redrawn()
            assert got["reads"].tobytes() == big["reads"][r0:r1_].tobytes() and got["geno"].tobytes() == big["geno"][p0:p1].tobytes()
            assert (got["reads"] != solo.reads).any()
    finally:
        one.close(); e.close()


def test_donor_mode_shares_one_genotype_per_snp_and_sample(m, pool):
    sp, g, pl, hyp, alpha, rho, a = pool
    cell, snp, nrd, start, _ = F.host_pairs(pl.cell_pair_off, pl.pair_snp, pl.pair_nrd)
    e = staged(m, g, pl)
    try:
        def table(**kw):
            e.redraw(hyp, alpha, rho, a, genotype_draw="donor", **kw)
            geno = e.get_redrawn()["geno"]
            tab = np.full((pl.n_snps, g.shape[1]), -1, dtype=np.int8)
            for s in range(2):
                ok = geno[:, s] >= 0
                v = hyp[cell[ok], s]
                seen = tab[snp[ok], v]
                tab[snp[ok], v] = geno[ok, s]
                again = tab[snp[ok], v]                                            # every pair at (SNP, sample) wrote the same value
                assert np.array_equal(again, geno[ok, s]) and ((seen < 0) | (seen == again)).all()
            return tab, e.get_redrawn()["reads"]
        t0, rd0 = table(seed=1, geno_seed=50)
        assert (t0 >= 0).sum() > 1500 and len(set(t0[t0 >= 0].tolist())) == 3
        t1, rd1 = table(seed=2, geno_seed=50, index_base=12345)
        assert np.array_equal(t0, t1) and (rd0 != rd1).any()                     # seed and index_base move the reads, not the genotypes
        t2, _ = table(seed=1, geno_seed=51)
        assert (t2 != t0).sum() > 100
    finally:
        e.close()


def run_results(e):
    e.run()
    llks, llk0s = e.get_singlet()
    _, l00, summ = e.get_doublet(want_grid=False)
    return llks, llk0s, l00, summ


def same_results(x, y):
    return all(u.tobytes() == w.tobytes() for u, w in zip(x, y))


def test_view_structure_and_adoption(m, pool):
    """The source staged as a device view of the test's own tensors: the redrawn view carries those very arrays and new reads; a second
    engine on the view gives the K1 / K2 bits of the host copy of get_redrawn."""
    sp, g, pl, hyp, alpha, rho, a = pool
    torch, capi = m["torch"], m["capi"]
    hs = pl.as_struct()
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(pl, k))).cuda() for k in ("cell_pair_off", "cell_read_off", "pair_snp", "pair_nrd")}
    t_reads = torch.zeros(len(pl.reads) + 64, dtype=torch.uint8, device="cuda")
    t_reads[:len(pl.reads)] = torch.from_numpy(pl.reads).cuda()
    ds = capi.Pileup(pl.n_cells, pl.n_snps, hs.n_pairs, hs.n_reads, t["cell_pair_off"].data_ptr(), t["cell_read_off"].data_ptr(), t["pair_snp"].data_ptr(),
                     t["pair_nrd"].data_ptr(), pl.pair_nrd.dtype.itemsize, capi.DMX_MEM_DEVICE, t_reads.data_ptr(), pl.rd_totl.ctypes.data,
                     pl.rd_pass.ctypes.data, pl.rd_uniq.ctypes.data)
    src = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    dev = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    hst = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    try:
        src.set_genotypes(g); src.set_pileup_struct(ds, keep=(t, t_reads))
        src.redraw(hyp, alpha, rho, a, seed=3, geno_seed=4, genotype_draw="donor")
        st = src.redrawn_pileup()
        assert st.memory == capi.DMX_MEM_DEVICE and (st.n_cells, st.n_snps, st.n_pairs, st.n_reads) == (pl.n_cells, pl.n_snps, hs.n_pairs, hs.n_reads)
        assert st.cell_pair_off == t["cell_pair_off"].data_ptr() and st.cell_read_off == t["cell_read_off"].data_ptr()
        assert st.pair_snp == t["pair_snp"].data_ptr() and st.pair_nrd == t["pair_nrd"].data_ptr() and st.nrd_width == hs.nrd_width
        assert st.reads and st.reads != t_reads.data_ptr() and not st.rd_totl
        assert torch.equal(t_reads[:len(pl.reads)].cpu(), torch.from_numpy(pl.reads))           # the source's reads are untouched
        got = src.get_redrawn()
        assert (got["reads"] != pl.reads).sum() > 100
        dev.set_genotypes(g); dev.set_pileup_struct(st, keep=src)
        host = m["engine"].HostPileup(pl.n_cells, pl.n_snps, pl.cell_pair_off, pl.cell_read_off, pl.pair_snp, pl.pair_nrd, got["reads"],
                                      pl.rd_totl, pl.rd_pass, pl.rd_uniq)
        hst.set_genotypes(g); hst.set_pileup(host)
        on_view, on_copy = run_results(dev), run_results(hst)
        assert same_results(on_view, on_copy)
        plain = staged(m, g, pl)
        try:
            assert not same_results(on_view, run_results(plain))
        finally:
            plain.close()
    finally:
        hst.close(); dev.close(); src.close()


def test_no_interference(m, pool):
    sp, g, pl, hyp, alpha, rho, a = pool
    e = staged(m, g, pl)
    try:
        before = run_results(e)
        f0 = e.fit_profile(hyp, alpha, rho, a, 4)
        e.redraw(hyp, alpha, rho, a, seed=9, geno_seed=9, genotype_draw="donor")
        got = [np.zeros_like(f0[k]) for k in ("obs", "mean", "var", "n_snp", "n_read", "n_trunc", "n_zero")]
        m["capi"].check(e._L.dmx_engine_get_fit(e._h, *(x.ctypes.data for x in got)))
        assert all(x.tobytes() == f0[k].tobytes() for x, k in zip(got, ("obs", "mean", "var", "n_snp", "n_read", "n_trunc", "n_zero")))
        llks, llk0s = e.get_singlet()
        _, l00, summ = e.get_doublet(want_grid=False)
        assert same_results(before, (llks, llk0s, l00, summ))
        assert same_results(before, run_results(e))                               # and the staged pileup itself is unchanged
    finally:
        e.close()


def test_the_law_on_the_device(m):
    """tests/test_redraw_cpu.py's pool and seeds: the device's PAIR-mode redraw, scored by the device's own fit_profile on a second engine."""
    sp, g, hyp, alpha, rho, a = R.law_pool(m["synth"], m["engine"].geno_from_gt)
    pl = host_pileup(m, sp)
    src = staged(m, g, pl)
    dst = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    try:
        info = src.redraw(hyp, alpha, rho, a, seed=R.LAW_SEED, geno_seed=R.LAW_GENO_SEED, genotype_draw="pair")
        dst.set_genotypes(g); dst.set_pileup_struct(src.redrawn_pileup(), keep=src)
        f = dst.fit_profile(hyp, alpha, rho, a, 4)
        reads = src.get_redrawn()["reads"]
    finally:
        dst.close(); src.close()
    idx, prob = R.marginal_first_read(sp, hyp, alpha, rho, a, g, m["mat"], m["err"])
    t_fit = R.fit_T(f, hyp[:, 0] >= 0)
    t_first = [R.first_read_T(sp, reads, idx, prob, directed=d) for d in (True, False)]
    print(f"device: fit T = {t_fit:+.3f}, first-read T = {t_first[0]:+.3f} (directed) {t_first[1]:+.3f} (plain); kernel {info['kernel_ms']:.3f} ms")
    assert info["n_reads_kept"] == 0 and info["n_pairs_drawn"] == len(idx)
    assert abs(t_fit) < 4.5, t_fit
    assert abs(t_first[0]) < 4.5 and abs(t_first[1]) < 4.5, t_first


def test_argument_and_state_errors(m):
    capi, eng = m["capi"], m["engine"]
    rng = np.random.default_rng(79)
    S, V, B = 100, 4, 20
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.3, 1.5, doublet_rate=0.0)
    pl = host_pileup(m, sp)
    a = rng.uniform(0.0, 1.0, size=S)
    hyp = np.stack([np.arange(B) % V, np.full(B, -1)], axis=1).astype(np.int32)
    al, rho = np.zeros(B), np.full(B, 0.1)

    def fails(e, code, *args, field=None, **kw):
        with pytest.raises(capi.DmxError) as ei:
            e.redraw(*args, **kw)
        assert ei.value.code == code, (ei.value.code, args, kw)
        named(str(ei.value), field)

    def named(msg, field=None):                                                 # the message names the entry point and the bad field
        assert "dmx_engine_redraw: " in msg and (field is None or field in msg), (msg, field)

    def queries_fail(e):
        for call in (e.redraw_info, e.redrawn_pileup, e.get_redrawn):
            with pytest.raises(capi.DmxError) as ei:
                call()
            assert ei.value.code == capi.DMX_ERR_STATE

    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.B, e.S = B, S
        fails(e, capi.DMX_ERR_STATE, hyp, al, rho, a)                           # neither genotypes nor a pileup yet
        e.set_genotypes(g)
        fails(e, capi.DMX_ERR_STATE, hyp, al, rho, a)                           # no pileup yet
        queries_fail(e)
        e.set_pileup(pl)
        queries_fail(e)                                                         # a query before a call
        for bad in (-0.1, 1.5, np.nan, np.inf):
            x = al.copy(); x[3] = bad
            fails(e, capi.DMX_ERR_ARG, hyp, x, rho, a, field="alpha[3]")
            x = rho.copy(); x[B - 1] = bad
            fails(e, capi.DMX_ERR_ARG, hyp, al, x, a, field=f"rho[{B - 1}]")
        for bad_a, field in ((np.full(S, 1.2), "ambient[0]"), (np.full(S, np.nan), "ambient[0]"), (a[:-1], "n_snps")):
            fails(e, capi.DMX_ERR_ARG, hyp, al, rho, bad_a, field=field)
        for bad_h in ((V, -1), (-2, -1), (0, V), (1, 1), (0, -2)):
            h = hyp.copy(); h[5] = bad_h
            fails(e, capi.DMX_ERR_ARG, h, al, rho, a, field="hyp[5]")
        fails(e, capi.DMX_ERR_ARG, hyp, al, rho, None, field="rho")             # rho without ambient
        fails(e, capi.DMX_ERR_ARG, hyp, al, rho, a, index_base=-1)
        with pytest.raises(ValueError):
            e.redraw(hyp, al, rho, a, genotype_draw="cell")
        with pytest.raises(ValueError):
            e.redraw(hyp[:-1], al, rho, a)
        rq = capi.RedrawRequest(B, S, capi.DMX_MEM_HOST, 2, hyp.ctypes.data, al.ctypes.data, None, None, 0, 0, 0)
        for fix in (dict(), dict(genotype_draw=-1), dict(genotype_draw=0, n_cells=B + 1), dict(n_cells=B, n_snps=S + 1), dict(n_snps=S, hyp_memory=7),
                    dict(hyp_memory=capi.DMX_MEM_HOST, hyp=None)):
            for k, v in fix.items():
                setattr(rq, k, v)
            assert e._L.dmx_engine_redraw(e._h, C.byref(rq)) == capi.DMX_ERR_ARG, fix
            named(e._L.dmx_last_error().decode())
        assert e._L.dmx_engine_redraw(e._h, None) == capi.DMX_ERR_ARG
        named(e._L.dmx_last_error().decode())
        assert e._L.dmx_engine_redraw_info(e._h, None) == capi.DMX_ERR_ARG
        queries_fail(e)                                                         # still nothing drawn
        info = e.redraw(hyp, al, rho, a)                                        # the defaults: donor draw, seeds 0
        assert info["genotype_draw"] == 1 and info["n_used"] == B and info["n_reads_drawn"] == len(pl.reads) - int(info["n_reads_kept"])
        good = e.get_redrawn()
        fails(e, capi.DMX_ERR_ARG, hyp, al, rho, a, index_base=-5)
        assert e.get_redrawn()["reads"].tobytes() == good["reads"].tobytes()    # a refused call leaves the last result readable
        capi.check(e._L.dmx_engine_get_redrawn(e._h, None, None))               # either pointer may be NULL
        assert e.redraw(hyp, al, None, a)["n_used"] == B                        # ambient without rho is fine: rho = 0
        st = e.redrawn_pileup()
        e.set_pileup(pl)                                                        # a new pileup: no result on it yet
        queries_fail(e)
        e.redraw(hyp, al, None, None)
        e.set_pileup_struct(e.redrawn_pileup(), keep=None)                      # an engine staged on its own redrawn pileup cannot redraw over it
        fails(e, capi.DMX_ERR_STATE, hyp, al, None, None)
        e.set_pileup(pl)
        par = np.stack([np.arange(B), np.full(B, -1)], axis=1).astype(np.int32)
        e.compose(par, np.full((B, 2), 1 << 32, dtype=np.uint64), 1)
        e.set_pileup_struct(e.composed_pileup(), keep=None)                     # nor over its own composed pileup
        fails(e, capi.DMX_ERR_STATE, hyp, al, None, None)
        assert st.reads
    finally:
        e.close()


def test_redraw_run_end_to_end(m, tmp_path, capsys):
    """redraw_run on fit.py's own scenario: 8 donors, one left out of the matrix, ~150 SNPs per barcode, 160 barcodes, 5 PAIR-mode
    replicates.  The five files have the stated headers and row counts; every cell of the missing donor has P.EMP = 1/6 (its observed Z is
    far below every null Z); the pooled null Z of the barcodes obeys |mean| sqrt(N) < 4.5 (a standard normal under the law PAIR mode draws
    from).  Nothing else is asserted about rates.  Measured once on the MI355X: SNG 700/700 and DBL 100/100 right; pooled null Z of the
    barcodes n 800, mean -0.0616, sd 1.028, 0.001 quantile -4.50 (|mean| sqrt(n) = 1.7); of the 1 446 SNPs with 10 or more cells n 7 230,
    mean -0.019, sd 1.043, 0.001 quantile -6.98."""
    D, refine, synth, eng = m["redraw"], m["refine"], m["synth"], m["engine"]
    sp, g, truth = F.dropped_donor_pool(np.random.default_rng(7), synth, lambda al: eng.geno_from_gt(al, 0.01), 1500, 8, 160, 0.1, 1.25)
    B, S, V = sp.n_cells, sp.n_snps, g.shape[1]
    pl = host_pileup(m, sp)
    samples = [f"S-{j}" for j in range(V)]
    barcodes = [synth.barcode_name(c) for c in range(B)]
    dump = tmp_path / "x.pileup.txt"
    refine.write_pileup_txt(str(dump), refine.PileupDump(samples, [(1, 100 + 10 * j, "A", "C") for j in range(S)], g, barcodes, pl))
    out = tmp_path / "rd"
    assert D.main(["--pileup", str(dump), "--out", str(out), "--reps", "5", "--genotype-draw", "pair", "--seed", "3"]) == 0
    print(capsys.readouterr().err)
    for ext in (".best", ".null.best", ".null.tsv", ".null_fit.tsv", ".null_sites.tsv", ".null_summary.tsv"):
        assert (tmp_path / ("rd" + ext)).exists(), ext
    rows = lambda ext: [l.split("\t") for l in (tmp_path / ("rd" + ext)).read_text().splitlines()]
    best, nbest = rows(".best"), rows(".null.best")
    assert nbest[0] == best[0] and len(nbest) == len(best) == B + 1
    null = rows(".null.tsv")
    assert "\t".join(null[0]) == D.NULL_HEADER.rstrip("\n") and len(null) == 5 * B + 1 and [r[0] for r in null[1::B]] == list("01234")
    fit_rows = rows(".null_fit.tsv")
    assert "\t".join(fit_rows[0]) == D.NULL_FIT_HEADER.rstrip("\n") and len(fit_rows) == B + 1
    assert [r[0].encode() for r in fit_rows[1:]] == sorted(b.encode() for b in barcodes)
    by_bc = {r[0]: r for r in fit_rows[1:]}
    missing = [c for c in range(B) if truth[c] < 0]
    assert len(missing) == 20
    for c in missing:
        assert abs(float(by_bc[barcodes[c]][5]) - 1.0 / 6.0) < 1e-5, by_bc[barcodes[c]]
    sites = rows(".null_sites.tsv")
    assert "\t".join(sites[0]) == D.NULL_SITES_HEADER.rstrip("\n") and len(sites) == S + 1 and all(len(r) == 10 for r in sites)
    summ = rows(".null_summary.tsv")
    assert "\t".join(summ[0]) == D.SUMMARY_HEADER.rstrip("\n") and [r[0] for r in summ[1:]] == ["SNG", "DBL", "#NULL", "#NULL.FIT", "#NULL.SITES"]
    n_hyp = {r[0]: int(r[1]) for r in summ[1:3]}
    assert n_hyp["SNG"] + n_hyp["DBL"] == 5 * B
    for r in summ[1:3]:
        assert int(r[1]) == sum(int(x) for x in r[2:])
    n, mean = int(summ[4][1]), float(summ[4][2])
    print(f"pooled null Z of the barcodes: n {n}, mean {mean:+.4f}, sd {summ[4][3]}, quantile {summ[4][4]}; sites: {summ[5][1:5]}")
    assert n == 5 * B and abs(mean) * np.sqrt(n) < 4.5, (n, mean)
