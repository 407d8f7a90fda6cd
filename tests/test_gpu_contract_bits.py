"""GPU (-m gpu): the feature kernels against the host emulator of their stated contracts, bit for bit.

include/dmx.h states, for the ambient profile, the ambient doublet profile, the goodness of fit, the genotype refinement, the cluster
stage / M-step, the share scan, the share fit (its Newton driver step by step) and the site audit, every operation and the order of
every sum.  tests/contract_emul.cpp restates those blocks as serial host loops (plain
recurrences and divisions, dmx_log's host emulation); tests/test_contract_emul_cpu.py shows, without a GPU, that the emulator computes
the right numbers, that these inputs tell a contracted product, a reversed sum and libm's log from the contract, and that no log
argument here is subnormal, inf or nan (those go to the runtime's log, which no host can promise to match).  Each case below runs the
engine once and the emulator once and compares the uint64 / uint32 views of every output.  gp' of the refinement and of the M-step goes
through the device's exp and stays on its 2-ulp tests (test_gpu_refine, test_gpu_cluster).

A difference is a finding: the failure message names the first differing element, which the emulator locates to a barcode, pair or
read on the CPU."""
import numpy as np
import pytest

import contract_emul as CE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m(tmp_path_factory):
    from demuxlet_amd import build, capi, engine, synth
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    mat, err = engine.phred_tables()
    return dict(engine=engine, emu=CE.build(tmp_path_factory.mktemp("contract_emul")), P=CE.problems(engine, synth), mat=mat, err=err)


def tables(m, p):
    return p.tables if p.tables is not None else (m["mat"], m["err"])


def staged(m, p, V=None, g=None):
    e = m["engine"].Engine(p.V if V is None else V, (0.0, 0.5), 0.5)
    if p.tables is not None:
        e.set_phred_tables(*p.tables)
    e.set_genotypes(p.g if g is None else g)
    sp = p.sp
    e.set_pileup(m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads,
                                        sp.rd_totl, sp.rd_pass, sp.rd_uniq))
    return e


def same_bits(what, got, want, nan_equal=False):
    """Every element's bits.  nan_equal (the share passes only): elements that are NaN on both sides count as equal — 0 / 0 gives a NaN whose
    sign and payload IEEE does not fix, and x86 and the device differ there; a NaN on one side only is a difference."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = CE.bits(got), CE.bits(want)
    ne = a != b
    if nan_equal:
        ne &= ~(np.isnan(got) & np.isnan(want))
    if ne.any():
        bad = np.argwhere(ne)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {a.size} elements differ; first at {i}: engine {got[i]!r} ({int(a[i]):#x}), "
                             f"emulator {want[i]!r} ({int(b[i]):#x})")


@pytest.mark.parametrize("case", CE.AMBIENT_CASES, ids=lambda c: f"{c[0]}-Q{c[1]}")
def test_ambient_profile_bits(m, case):
    name, Q = case
    p = m["P"][name]
    assign, a, grid = CE.assignment(p), CE.amb_freq(p), CE.GRIDS[Q]
    e = staged(m, p)
    try:
        ll, n_snp, n_read = e.ambient_profile(assign, a, grid)
    finally:
        e.close()
    LL, ns, nr, cnt = m["emu"].ambient(p.sp, p.g, *tables(m, p), assign, a, grid)
    assert cnt["log_other"] == 0
    same_bits("n_snp", n_snp, ns); same_bits("n_read", n_read, nr); same_bits("LL[B][Q]", ll, LL)
    assert not ll[assign < 0].any()                                          # unassigned barcodes: zero rows


@pytest.mark.parametrize("case", CE.AMBIENT_DBL_CASES, ids=lambda c: f"{c[0]}-C{c[1]}-A{c[2]}-Q{c[3]}")
def test_ambient_doublet_profile_bits(m, case):
    name, Cn, A, Q = case
    p = m["P"][name]
    cand, alphas, a, grid = CE.candidates(p, Cn), CE.ALPHAS[A], CE.amb_freq(p), CE.GRIDS[Q]
    e = staged(m, p)
    try:
        ll, n_snp, n_read = e.ambient_doublet_profile(cand, alphas, a, grid)
        info = e.ambient_doublet_info()
    finally:
        e.close()
    # the slot count alone picks the instantiation (dmx_engine_ambient_doublet: 1, 2, 3-4, 5-8 slots)
    assert info["n_cand"] == Cn and info["n_alpha"] == A and info["n_grid"] == Q and info["n_used"] == int((cand[:, :, 0] >= 0).sum())
    LL, ns, nr, cnt = m["emu"].ambient_doublet(p.sp, p.g, *tables(m, p), cand, alphas, a, grid)
    assert cnt["log_other"] == 0
    same_bits("n_snp", n_snp, ns); same_bits("n_read", n_read, nr); same_bits("LL[B][C][A][Q]", ll, LL)


@pytest.mark.parametrize("case", CE.FIT_CASES, ids=lambda c: f"{c[0]}-M{c[1]}-{'soup' if c[2] else 'clean'}")
def test_fit_profile_bits(m, case):
    name, M, soup = case
    p = m["P"][name]
    hyp, alpha, rho = CE.hypotheses(p)
    a = CE.amb_freq(p)
    e = staged(m, p)
    try:
        out = e.fit_profile(hyp, alpha, rho if soup else None, a if soup else None, M)
    finally:
        e.close()
    want, cnt = m["emu"].fit(p.sp, p.g, *tables(m, p), hyp, alpha, rho if soup else None, a if soup else None, M)
    assert cnt["log_other"] == 0 and cnt["log_zero"] == 0
    for k in ("n_snp", "n_read", "n_trunc", "n_zero", "obs", "mean", "var"):
        same_bits(k, out[k], want[k])
    if p.V > 1:
        assert ((hyp[:, 0] >= 0) & (hyp[:, 1] < 0)).any() and (hyp[:, 1] >= 0).any()          # both kernels ran


@pytest.mark.parametrize("name", CE.REFINE_CASES)
def test_refinement_and_stage_bits(m, name):
    p = m["P"][name]
    assign = CE.refine_assignment(p)
    e = staged(m, p)
    try:
        ll, n_cell, n_ref, n_alt, _ = e.refine_genotypes(assign, p.g, 1e-3)
        e.cluster_stage()
        off, cell, lgl, s_ref, s_alt = e.get_cluster_stage()
    finally:
        e.close()
    LL, nc, nr, na, cnt = m["emu"].refine(p.sp, p.g.shape[0], p.V, *tables(m, p), assign)
    assert cnt["log_other"] == 0 and cnt["log_zero"] == 0
    same_bits("n_cell", n_cell, nc); same_bits("n_ref", n_ref, nr); same_bits("n_alt", n_alt, na); same_bits("LL[S][V][3]", ll, LL)
    roff, rcell, rlgl, ra, _ = m["emu"].cluster_stage(p.sp, *tables(m, p))
    same_bits("snp_off", off, roff); same_bits("cell", cell, rcell)
    same_bits("n_ref per slot", s_ref, (ra & 0xFFFF).astype(np.int64)); same_bits("n_alt per slot", s_alt, (ra >> 16).astype(np.int64))
    same_bits("lgl[P][3]", lgl, rlgl)


@pytest.mark.parametrize("case", CE.MSTEP_CASES, ids=lambda c: f"{c[0]}-C{c[1]}")
def test_cluster_mstep_bits(m, case):
    name, Cn = case
    p = m["P"][name]
    S = p.sp.n_snps
    w = CE.mstep_weights(p, Cn)
    q = np.tile(np.array([0.25, 0.5, 0.25], dtype=np.float32), (S, 1))
    e = staged(m, p, V=Cn, g=np.full((S, Cn, 3), 1 / 3, dtype=np.float32))
    try:
        e.cluster_stage()
        off, cell, lgl = e.get_cluster_stage()[:3]
        LL, W, _ = e.cluster_mstep(w, q, 1e-3)
    finally:
        e.close()
    roff, rcell, rlgl, _, _ = m["emu"].cluster_stage(p.sp, *tables(m, p))
    same_bits("snp_off", off, roff); same_bits("cell", cell, rcell); same_bits("lgl[P][3]", lgl, rlgl)
    RL, RW = m["emu"].cluster_mstep(roff, rcell, rlgl, w)
    same_bits("W[S][C]", W, RW); same_bits("LL[S][C][3]", LL, RL)


def soup(p, given):
    return (CE.barcode_rho(p), CE.amb_freq(p)) if given else (None, None)


@pytest.mark.parametrize("case", CE.SHARE_SCAN_CASES, ids=lambda c: f"{c[0]}-T{c[1]}-{'soup' if c[2] else 'clean'}")
def test_share_scan_bits(m, case):
    name, T, given = case
    p = m["P"][name]
    an = CE.anchors(p, T)
    rho, a = soup(p, given)
    e = staged(m, p)
    try:
        out, n_snp, n_read = e.share_scan(an, rho, a)
        info = e.share_info()
    finally:
        e.close()
    assert info["have_scan"] == 1 and info["n_anchor"] == T and info["n_samples"] == p.V
    assert info["scan_entries"] == int((an >= 0).sum()) * (p.V - 1)
    want, nsr, cnt = m["emu"].share_scan(p.sp, p.g, *tables(m, p), an, rho, a)
    assert cnt["log_other"] == 0 and (cnt["log_zero"] > 0) == (name == "zero")
    same_bits("n_snp_read[B][T][2]", np.stack([n_snp, n_read], axis=2), nsr)
    same_bits("out[B][T][V][3]", out, want, nan_equal=True)


IDENTITY_PROBLEMS = ("pool_02", "mix_full", "mix_edges", "panel_66", "dense_64", "edge", "zero")


def identity_scan(p, cand):
    """(anchors[B][T], the barcodes of at most 64 pairs): slot t < min(C, 4) of the scan holds v1 of the fit's slot t."""
    T = min(cand.shape[1], 4)
    return np.ascontiguousarray(cand[:, :T, 0]), np.flatnonzero(np.diff(p.sp.cell_pair_off) <= 64)


@pytest.mark.parametrize("case", CE.SHARE_FIT_CASES, ids=CE.share_fit_id)
def test_share_fit_bits(m, case):
    name, Cn, start, tol, max_iter, probe, given = case
    p = m["P"][name]
    cand = CE.share_candidates(p, Cn)
    rho, a = soup(p, given)
    e = staged(m, p)
    try:
        fit = e.share_fit(cand, rho, a, start=start, tol=tol, max_iter=max_iter, probe=probe)
        info = e.share_info()
        an, short = identity_scan(p, cand)
        scan = e.share_scan(an, rho, a)[0] if name in IDENTITY_PROBLEMS else None
    finally:
        e.close()
    used = cand[:, :, 0] >= 0
    assert info["have_fit"] == 1 and info["n_cand"] == Cn and info["fit_used"] == int(used.sum())
    assert info["fit_evals"] == int(fit["n_eval"][used].sum()) + (int(used.sum()) if probe >= 0 else 0)
    val, cts, _, cnt = m["emu"].share_fit(p.sp, p.g, *tables(m, p), cand, rho, a, start, tol, max_iter, probe)
    assert cnt["log_other"] == 0 and (cnt["log_zero"] > 0) == (name == "zero")
    same_bits("counts[B][C][4]", np.stack([fit[k] for k in CE.SHARE_COUNTS], axis=2), cts)
    same_bits("values[B][C][13]", np.stack([fit[k] for k in CE.SHARE_VALUES], axis=2), val, nan_equal=True)
    if scan is not None:
        # a barcode of at most 64 pairs leaves at most one term in each of the fit's 64 sums: its evaluation at 0 is the scan's serial sum
        for b in short:
            for t in range(an.shape[1]):
                if an[b, t] >= 0:
                    at0 = np.array([fit[k][b, t] for k in ("ll0", "d10", "d20")])
                    same_bits(f"the fit at 0 against the scan, barcode {b} slot {t}", at0, scan[b, t, cand[b, t, 1]], nan_equal=True)


def site_arguments(p, case):
    _, M, given, lists = case
    hyp, alpha, rho = CE.site_hypotheses(p, lists)
    return hyp, alpha, rho if given else None, CE.amb_freq(p) if given else None, M


@pytest.mark.parametrize("case", CE.SITE_CASES, ids=CE.site_id)
def test_site_fit_bits(m, case):
    p = m["P"][case[0]]
    hyp, alpha, rho, a, M = site_arguments(p, case)
    S = p.g.shape[0]
    e = staged(m, p)
    try:
        out = e.site_fit(hyp, alpha, rho, a, M)
        info = e.site_fit_info()
        if case == CE.SITE_WAVES_CASE:                  # one chunk per wave of the partial buffer: the bits must not move
            waves = e.site_fit(hyp, alpha, rho, a, M, partial_bytes=64 * S)
            winfo = e.site_fit_info()
    finally:
        e.close()
    ns, nd = int(((hyp[:, 0] >= 0) & (hyp[:, 1] < 0)).sum()), int(((hyp[:, 0] >= 0) & (hyp[:, 1] >= 0)).sum())
    assert (info["n_singlet"], info["n_doublet"], info["n_used"], info["max_reads"]) == (ns, nd, ns + nd, M)
    assert info["n_chunks"] == -(-ns // 64) + -(-nd // 64) and info["chunk_cells"] == 64
    want, cnt = m["emu"].site_fit(p.sp, p.g, *tables(m, p), hyp, alpha, rho, a, M)
    assert cnt["log_other"] == 0 and cnt["log_zero"] == 0
    for k in CE.SITE_COUNTS + CE.SITE_FLOATS:
        same_bits(k, out[k], want[k])
    assert info["n_zero"] == int(want["n_zero"].sum()) and info["n_trunc"] == int(want["n_trunc"].sum())
    if case == CE.SITE_WAVES_CASE:
        assert winfo["n_waves"] == winfo["n_chunks"] == info["n_chunks"] and info["n_waves"] == 1
        for k in CE.SITE_COUNTS + CE.SITE_FLOATS:
            same_bits(k + " at one chunk per wave", waves[k], want[k])
