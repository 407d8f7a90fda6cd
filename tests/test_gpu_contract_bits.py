"""GPU (-m gpu): the feature kernels against the host emulator of their stated contracts, bit for bit.

include/dmx.h states, for the ambient profile, the ambient doublet profile, the goodness of fit, the genotype refinement and the cluster
stage / M-step, every operation and the order of every sum.  tests/contract_emul.cpp restates those blocks as serial host loops (plain
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


def same_bits(what, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = CE.bits(got), CE.bits(want)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
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
