"""GPU (-m gpu): empirical-Bayes priors from the doublet grid (Engine.prior_step / prior_fit / prior_call, prior.prior_run; DESIGN.md
section 25) against the numpy restatement tests/prior_ref.py.

Bounds.  N_j, the two masses and E_b: relative 1e-9 (E_b through |log E_b - ref| <= 1e-9, which is that bound without forming
exp(1e5)); log E_b and LL: 1e-9 max(1, |value|).  Forming L + log w - m at |L| <= 1e5 costs a few ulp(1e5) ~ 4e-11 relative per term and
every sum is of non-negative terms.  Below 1e-300 a float64 is close to the subnormal range and no longer carries a relative 1e-9, so
values are compared with an absolute floor of 1e-300 beside the relative bound."""
import numpy as np
import pytest

import prior_pool as P
import prior_ref as R

pytestmark = pytest.mark.gpu

ALPHAS = {2: (0.0, 0.5), 3: (0.0, 0.25, 0.5), 4: (0.0, 0.1, 0.25, 0.5)}
RTOL, TINY = 1e-9, 1e-300


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import build, capi, engine, prior, synth
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return dict(torch=torch, capi=capi, engine=engine, prior=prior, synth=synth)


def host_pileup(m, sp):
    return m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads,
                                  sp.rd_totl, sp.rd_pass, sp.rd_uniq)


def random_grid(rng, B, V, A):
    """Barcodes of three kinds (singlet-dominant, doublet-dominant, mixed) at offsets up to 1e5, with spreads of 1, 30 and 2000 (the last
    far beyond exp's 745: most terms are exactly 0) and a sprinkle of -inf entries."""
    g = np.empty((B, V, V, A))
    for b in range(B):
        scale = (1.0, 30.0, 2000.0)[b % 3]
        x = -scale * rng.random((V, V, A)) - 1e5 * rng.random() * (b % 5 != 0)
        kind = (b // 3) % 3
        if kind == 0:
            x[rng.integers(V), 0, 0] += 3.0 * scale
        elif kind == 1:
            j = rng.integers(V); k = (j + 1 + rng.integers(V - 1)) % V
            x[j, k, 1 + rng.integers(A - 1)] += 3.0 * scale
        if b % 7 == 3:
            x[rng.random((V, V, A)) < 0.05] = -np.inf
        g[b] = x
    return g


def random_pi(rng, V, zeros=True):
    pi = rng.random(V) + 0.05
    if zeros and V >= 3:
        z = rng.permutation(V)[:max(1, V // 5)]
        pi[z] = 0.0
    return pi / pi.sum()


def close(a, b):
    return np.allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=RTOL, atol=TINY)


def close_log(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= 1e-9 * np.maximum(1.0, np.abs(b))))


def check_step(s, ref, V):
    assert np.array_equal(s["flags"], ref["flags"])
    assert s["b_in"] == ref["b_in"]
    assert close(s["rows"][:, :V + 2], ref["rows"][:, :V + 2])
    assert bool(np.all(np.abs(s["rows"][:, V + 2] - ref["log_e"]) <= 1e-9))      # E_b within relative 1e-9
    assert close_log(s["rows"][:, V + 2], ref["log_e"])
    assert close(s["N"], ref["N"]) and close(s["hom"], ref["hom"]) and close(s["het"], ref["het"])
    assert close_log(s["ll"], ref["ll"])


SHAPES = [(2, 2, 1), (2, 3, 200), (3, 4, 63), (3, 2, 64), (16, 3, 65), (16, 2, 200), (17, 4, 1), (17, 2, 63), (33, 3, 64), (33, 4, 65),
          (64, 2, 200), (64, 4, 63), (65, 2, 65), (65, 3, 64)]


@pytest.mark.parametrize("V,A,B", SHAPES)
def test_step_against_restatement(m, V, A, B):
    rng = np.random.default_rng(V * 1000 + A * 100 + B)
    grid = random_grid(rng, B, V, A)
    e = m["engine"].Engine(V, ALPHAS[A])
    try:
        for d, zeros in ((0.0, True), (0.2, True), (1.0, False), (0.2, False)):
            pi = random_pi(rng, V, zeros)
            ref = R.step(grid, pi, d)
            assert ref["b_in"] > 0
            s = e.prior_step(pi, d, grid=grid, rows=True)
            print(V, A, B, d, "b_in", s["b_in"], "max |dlogE|", float(np.abs(s["rows"][:, V + 2] - ref["log_e"]).max()),
                  "N rel", float(np.max(np.abs(s["N"] - ref["N"]) / np.maximum(np.abs(ref["N"]), TINY))))
            check_step(s, ref, V)
            if zeros and V >= 3:
                assert (s["N"][pi == 0] == 0).all() and (s["rows"][:, :V][:, pi == 0] == 0).all()      # exact zeros stay exact
            if d == 0.0:
                assert s["het"] == 0.0 and s["hom"] == 0.0
    finally:
        e.close()


def serial_sum(x):
    t = 0.0
    for v in np.asarray(x, dtype=np.float64):
        t = t + v
    return t


def test_bits(m):
    torch = m["torch"]
    V, A, B = 17, 3, 200
    rng = np.random.default_rng(11)
    grid = random_grid(rng, B, V, A)
    grid[5, 2, 3, 1] = np.nan
    mask = np.ones(B, dtype=np.uint8); mask[[0, 64, 130]] = 0
    pi, d = random_pi(rng, V), 0.2
    e = m["engine"].Engine(V, ALPHAS[A])
    try:
        s = e.prior_step(pi, d, grid=grid, mask=mask, rows=True)
        assert s["flags"][5] == R.BAD and (s["flags"][[0, 64, 130]] == R.MASKED).all() and s["b_in"] == B - 4
        # the fold: the included rows in chunks of 64, bit for bit; then the M-step
        tot = R.fold_chunked(s["rows"], s["flags"])
        assert np.array_equal(tot[:V], s["N"]) and tot[V] == s["hom"] and tot[V + 1] == s["het"] and tot[V + 2] == s["ll"]
        assert np.array_equal(s["pi_next"], s["N"] / serial_sum(s["N"]))
        assert s["d_next"] == min((s["hom"] + s["het"]) / float(s["b_in"]), 1.0)
        # again, and on a caller's stream
        s2 = e.prior_step(pi, d, grid=grid, mask=mask, rows=True)
        st = torch.cuda.Stream()
        e.set_stream(st.cuda_stream)
        s3 = e.prior_step(pi, d, grid=grid, mask=mask, rows=True)
        e.set_stream(0)
        # the grid in device memory
        tg = torch.from_numpy(grid).cuda()
        torch.cuda.synchronize()
        s4 = e.prior_step(pi, d, grid=int(tg.data_ptr()), n_cells=B, mask=mask, rows=True)
        for o in (s2, s3, s4):
            assert o["rows"].tobytes() == s["rows"].tobytes() and o["N"].tobytes() == s["N"].tobytes()
            assert (o["ll"], o["hom"], o["het"], o["d_next"]) == (s["ll"], s["hom"], s["het"], s["d_next"])
            assert o["pi_next"].tobytes() == s["pi_next"].tobytes()
        # a barcode alone
        for b in (1, 63, 66, 199):
            one = e.prior_step(pi, d, grid=grid[b:b + 1], rows=True)
            assert one["rows"][0].tobytes() == s["rows"][b].tobytes()
        # the other barcodes of a chunk in another order, and fewer of them
        perm = np.arange(B); perm[1:60] = perm[1:60][::-1]
        sp = e.prior_step(pi, d, grid=grid[perm], mask=mask[perm], rows=True)
        assert sp["rows"][[0, 60, 61, 199]].tobytes() == s["rows"][[0, 60, 61, 199]].tobytes()
        assert sp["rows"][30].tobytes() == s["rows"][perm[30]].tobytes()
        # the records do not depend on the company either
        c = e.prior_call(pi, d, grid=grid, mask=mask)
        c1 = e.prior_call(pi, d, grid=grid[7:9])
        assert c[7:9].tobytes() == c1.tobytes()
        assert np.array_equal(c["log_e"], s["rows"][:, V + 2]) and np.array_equal(c["p_het"], s["rows"][:, V + 1])
        # a call never touches a step's rows or flags, whatever its barcode count (more barcodes: its buffers grow)
        s5 = e.prior_step(pi, d, grid=grid, mask=mask, rows=True)
        big = np.concatenate([grid[::-1], grid, grid])
        cb = e.prior_call(pi, d, grid=big)
        assert len(cb) == 3 * B and cb["flag"][B - 1 - 5] == R.BAD and cb["flag"][0] == 0
        kept = e.get_prior_step(rows=True)
        assert kept["flags"].tobytes() == s["flags"].tobytes() and kept["rows"].tobytes() == s["rows"].tobytes()
        assert kept["N"].tobytes() == s5["N"].tobytes() and kept["ll"] == s["ll"] and kept["b_in"] == s["b_in"]
        e.prior_fit(grid=grid[:10], max_iter=2, tol=0.0)     # a fit overwrites the rows: the step's results are gone
        with pytest.raises(m["capi"].DmxError) as ei:
            e.get_prior_step()
        assert ei.value.code == m["capi"].DMX_ERR_STATE
    finally:
        e.close()


def structured_grid(rng, B, V, A, shares, rate, depth=25.0):
    """Grids that look like a pool's: every barcode has a true singlet or pair whose entries stand `depth` above the others."""
    g = -depth * (1.0 + rng.random((B, V, V, A))) - 40.0 * rng.random((B, 1, 1, 1))
    first = rng.choice(V, size=B, p=shares)
    second = rng.choice(V, size=B, p=shares)
    dbl = rng.random(B) < rate
    for b in range(B):
        j, k = int(first[b]), int(second[b])
        if dbl[b] and j != k:
            g[b, j, k, 1:] += depth; g[b, k, j, 1:] += depth
            g[b, j, 0, 0] += 0.6 * depth; g[b, k, 0, 0] += 0.6 * depth
        else:
            g[b, j, 0, 0] += depth
            g[b, j, :, 1:] += 0.7 * depth; g[b, :, j, 1:] += 0.7 * depth
    return g


def test_fit(m):
    """25 iterations at tol = 0, GPU against restatement.  The bound on pi and d is max(1e-9, 100 x drift), drift = the largest
    difference between the restatement's float64 and longdouble runs over the same 25 iterations on these grids, computed here; measured
    on x86-64 (80-bit longdouble): 2.8e-16 on these grids, so the bound is 1e-9 (the GPU's fit was 4.4e-16 away from the float64 run)."""
    V, A, B = 6, 3, 300
    rng = np.random.default_rng(21)
    shares = np.array([0.4, 0.25, 0.2, 0.1, 0.05, 0.0])
    grid = structured_grid(rng, B, V, A, shares, 0.2, depth=6.0)
    f64 = R.fit(grid, None, 0.1, 25, 0.0)
    fld = R.fit(grid, None, 0.1, 25, 0.0, longdouble=True)
    drift = max(float(np.abs(f64["pi"] - fld["pi"]).max()), abs(float(f64["d"] - fld["d"])))
    bound = max(1e-9, 100.0 * drift)
    e = m["engine"].Engine(V, ALPHAS[A])
    try:
        f = e.prior_fit(grid=grid, d0=0.1, max_iter=25, tol=0.0)
        print("fit: drift", drift, "bound", bound, "gpu-ref", float(np.abs(f["pi"] - f64["pi"]).max()), abs(f["d"] - float(f64["d"])),
              "pi", f["pi"], "d", f["d"])
        assert f["n_iter"] == 25 and not f["converged"] and f["b_in"] == B
        assert np.abs(f["pi"] - f64["pi"]).max() <= bound and abs(f["d"] - float(f64["d"])) <= bound
        assert close_log(f["ll_trace"], f64["ll_trace"]) and np.abs(f["d_trace"] - f64["d_trace"].astype(np.float64)).max() <= bound
        # one restatement step from the GPU's final (pi, d) reproduces the GPU's own last step
        ref = R.step(grid, f["pi"], f["d"])
        assert close(f["N"], ref["N"]) and close(f["hom"], ref["hom"]) and close(f["het"], ref["het"]) and close_log(f["ll"], ref["ll"])
        # the stop rule
        g = e.prior_fit(grid=grid, d0=0.1, max_iter=200, tol=1e-6)
        r = R.fit(grid, None, 0.1, 200, 1e-6)
        assert g["converged"] and 2 <= g["n_iter"] < 200
        assert g["ll_trace"][-1] - g["ll_trace"][-2] < 1e-6 * B and (np.diff(g["ll_trace"])[:-1] >= 1e-6 * B).all()
        assert abs(g["n_iter"] - r["n_iter"]) <= 1 and np.abs(g["pi"] - r["pi"]).max() < 1e-5
        # held shares, held rate
        h = e.prior_fit(grid=grid, d0=0.3, max_iter=5, tol=0.0, fix_d=True)
        assert h["d"] == 0.3 and (h["d_trace"] == 0.3).all()
        h = e.prior_fit(grid=grid, pi0=shares + 0.01, d0=0.3, max_iter=5, tol=0.0, fix_pi=True)
        assert np.array_equal(h["pi"], (shares + 0.01) / serial_sum(shares + 0.01)) and h["d"] != 0.3
        inf = e.prior_info()
        assert inf["n_iter"] == 5 and inf["bytes_per_iter"] == grid.nbytes and inf["estep_ms"] > 0 and inf["fold_ms"] > 0
    finally:
        e.close()


def check_calls(c, ref, V, A):
    ok = ref["flag"] == 0
    assert np.array_equal(c["flag"], ref["flag"])
    for n in ("p_sng", "p_het", "p_hom", "p_sng1", "p_sng2", "p_dbl1"):
        assert np.abs(c[n] - np.asarray(ref[n], dtype=np.float64)).max() <= 1e-9, n
    assert close_log(c["log_e"], ref["log_e"])
    assert (c["i_sng1"][~ok] == -1).all() and (c["j_dbl"][~ok] == -1).all()
    xS, xD = ref["xS"], ref["xD"]
    for b in np.flatnonzero(ok):
        for name in ("i_sng1", "i_sng2"):
            got, want = int(c[name][b]), int(ref[name][b])
            if got != want:                          # a near-tie: the device's choice is as good as the restatement's within 1e-9
                assert xS[b, got] >= xS[b, want] - 1e-9, (b, name)
        assert c["i_sng1"][b] != c["i_sng2"][b]
        got = (int(c["j_dbl"][b]), int(c["k_dbl"][b]), int(c["n_dbl"][b]))
        want = (int(ref["j_dbl"][b]), int(ref["k_dbl"][b]), int(ref["n_dbl"][b]))
        if got != want:
            assert want[0] >= 0 and got[0] >= 0 and got[0] != got[1] and got[2] >= 1
            assert xD[b][got[0], got[1], got[2] - 1] >= xD[b][want[0], want[1], want[2] - 1] - 1e-9, b


@pytest.mark.parametrize("V,A,B", [(3, 2, 40), (16, 3, 65), (65, 2, 20), (33, 4, 30)])
def test_calls(m, V, A, B):
    rng = np.random.default_rng(V + A + B)
    grid = random_grid(rng, B, V, A)
    grid[0] = -np.inf                               # a bad barcode
    # exact ties: duplicate singlet entries and duplicate doublet entries (the first maximum must win)
    grid[1, :, 0, 0] = -5.0
    grid[1, :, :, 1:] = -7.0
    grid[2, :, 0, 0] = -9.0
    grid[2, V - 1, 0, 0] = grid[2, 1, 0, 0] = -3.0
    grid[2, :, :, 1:] = -50.0
    grid[2, 2, 1, A - 1] = grid[2, 1, 2, A - 1] = grid[2, 1, 2, 1] = -1.0 if A == 2 else -1.5
    mask = np.ones(B, dtype=np.uint8); mask[B - 1] = 0
    e = m["engine"].Engine(V, ALPHAS[A])
    try:
        for d, pi in ((0.2, np.full(V, 1.0 / V)), (0.2, random_pi(rng, V)), (0.0, random_pi(rng, V, False)), (1.0, random_pi(rng, V))):
            c = e.prior_call(pi, d, grid=grid, mask=mask)
            ref = R.call(grid, pi, d, mask)
            check_calls(c, ref, V, A)
            if pi[0] == pi[1] == pi[V - 1] and d == 0.2:
                # uniform shares leave the ties exact: indices must be the restatement's (first maximum)
                for n in ("i_sng1", "i_sng2", "j_dbl", "k_dbl", "n_dbl"):
                    assert np.array_equal(c[n][1:3], ref[n][1:3]), n
                assert (c["i_sng1"][1], c["i_sng2"][1], c["j_dbl"][1], c["k_dbl"][1], c["n_dbl"][1]) == (0, 1, 0, 1, 1)
                assert (c["i_sng1"][2], c["i_sng2"][2], c["j_dbl"][2], c["k_dbl"][2]) == (1, V - 1, 1, 2)
            if d == 0.0:
                assert (c["j_dbl"] == -1).all() and (c["p_dbl1"] == 0).all() and (c["p_het"] == 0).all()
        assert e.prior_info()["call_ms"] > 0
    finally:
        e.close()


@pytest.fixture(scope="module")
def staged(m):
    """A small real pileup after run_doublet: V = 8, 200 barcodes (a few without pairs), the default grid, doublet prior 0.5."""
    V, S, B = 8, 300, 200
    rng = np.random.default_rng(31)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.01, 1.5)
    g = m["engine"].geno_from_gt(raw.alleles, 0.01).reshape(S, V, 3)
    e = m["engine"].Engine(V, (0.0, 0.5), 0.5)
    e.set_genotypes(g)
    e.set_pileup(host_pileup(m, sp))
    e.run_singlet()
    e.run_doublet()
    yield dict(e=e, sp=sp, V=V, B=B, g=g)
    e.close()


def test_uniform_priors_reproduce_the_reference_posterior(m, staged):
    e, V, B = staged["e"], staged["V"], staged["B"]
    def everything_else():
        """Every result the engine held before the pass, as bytes: the singlet stage, the grid, llks00, K3's records, the singlet column,
        a gather of cell grids, the device-formatted .pair text of a few barcodes and the kernel names of the last run."""
        llks, llk0s = e.get_singlet()
        grid, l00, summ = e.get_doublet()
        cells = np.flatnonzero(np.diff(staged["sp"].cell_pair_off) > 0)[[0, 3, -1]].astype(np.int32)
        txt = e.format_pair(cells, [f"c{i}" for i in cells], [f"s{j}" for j in range(V)])
        pair_text = txt[0] + txt[1].tobytes() + txt[2].tobytes() + repr(txt[3]).encode()
        names = e.kernel_names()
        return dict(llks=llks.tobytes(), llk0s=llk0s.tobytes(), grid=grid.tobytes(), l00=l00.tobytes(), summary=summ.tobytes(),
                    sing=e.get_sing().tobytes(), cell_grids=e.get_cell_grids(cells).tobytes(), pair_text=pair_text,
                    names=repr(sorted(names.items())))
    before = everything_else()
    grid0, l000, sum0 = e.get_doublet()
    npairs = np.diff(staged["sp"].cell_pair_off)
    assert (npairs == 0).any() and (npairs > 0).sum() > 150
    d = m["prior"].uniform_rate(0.5, V)
    t = 0.5 / (2 * (V - 1) * 0.5)
    assert d == t * V / (1 + t * (V - 1))
    pi = np.full(V, 1.0 / V)
    c = e.prior_call(pi, d)
    s = e.prior_step(pi, d, rows=True)
    has = npairs > 0
    assert np.array_equal(c["flag"] == 0, has) and (c["flag"][~has] == R.MASKED).all() and s["b_in"] == int(has.sum())
    want = sum0["sum_double"] / (sum0["sum_single"] + sum0["sum_double"])
    print("PRB.HET against K3: max diff", float(np.abs(c["p_het"][has] - want[has]).max()))
    assert np.abs(c["p_het"][has] - want[has]).max() <= 1e-9
    assert np.abs(s["rows"][has, V + 1] - want[has]).max() <= 1e-9
    # the engine's own grid, its host copy and a fit leave the same bits; every other result of the engine stays
    s_host = e.prior_step(pi, d, grid=grid0, mask=has, rows=True)
    assert s_host["rows"].tobytes() == s["rows"].tobytes() and s_host["ll"] == s["ll"] and s_host["N"].tobytes() == s["N"].tobytes()
    e.prior_fit(max_iter=5, tol=0.0)
    after = everything_else()
    for k in before:
        assert after[k] == before[k], k


def test_masks_and_bad_barcodes(m, staged):
    e, V, B = staged["e"], staged["V"], staged["B"]
    grid, _, _ = e.get_doublet()
    npairs = np.diff(staged["sp"].cell_pair_off)
    has = npairs > 0
    pi, d = np.full(V, 1.0 / V), 0.15
    base = e.prior_step(pi, d, rows=True)
    assert np.array_equal(base["flags"] == R.MASKED, ~has) and (base["rows"][~has] == 0).all()
    ref = R.step(grid, pi, d, has)
    check_step(base, ref, V)
    mask = has.copy(); mask[np.flatnonzero(has)[:10]] = False
    s = e.prior_step(pi, d, mask=mask, rows=True)
    assert s["b_in"] == int(mask.sum()) and np.array_equal(s["flags"] == 0, mask)
    assert s["rows"][mask].tobytes() == base["rows"][mask].tobytes()
    check_step(s, R.step(grid, pi, d, mask), V)
    bad = grid.copy()
    b0, b1, b2 = np.flatnonzero(has)[[20, 21, 22]]
    bad[b0, 1, 2, 1] = np.nan                        # a used entry
    bad[b1] = -np.inf
    bad[b2, 3, 3, 1] = np.nan                        # the diagonal and the column [j][k != 0][0] are never read into a result
    bad[b2, 3, 2, 0] = np.nan
    s = e.prior_step(pi, d, grid=bad, mask=has, rows=True)
    assert s["flags"][b0] == R.BAD and s["flags"][b1] == R.BAD and s["flags"][b2] == 0 and s["b_in"] == int(has.sum()) - 2
    assert (s["rows"][[b0, b1]] == 0).all() and s["rows"][b2].tobytes() == base["rows"][b2].tobytes()
    check_step(s, R.step(bad, pi, d, has), V)
    c = e.prior_call(pi, d, grid=bad, mask=has)
    assert c["flag"][b0] == R.BAD and c["p_het"][b0] == 0 and c["i_sng1"][b0] == -1 and np.isfinite(c["log_e"]).all()
    f = e.prior_fit(grid=bad, mask=has, max_iter=3, tol=0.0)
    assert f["b_in"] == int(has.sum()) - 2 and np.isfinite(f["ll"]) and np.isfinite(f["pi"]).all()


def test_argument_and_state_errors(m, staged):
    import ctypes as C
    capi, eng = m["capi"], m["engine"]
    V = 4
    grid = -np.random.default_rng(5).random((3, V, V, 2))
    pi = np.full(V, 0.25)
    e = eng.Engine(V, (0.0, 0.5))
    try:
        def code(fn, *a, **k):
            with pytest.raises(capi.DmxError) as ei:
                fn(*a, **k)
            return ei.value.code
        assert code(e.prior_info) == capi.DMX_ERR_STATE
        assert code(e.get_prior_step) == capi.DMX_ERR_STATE
        out = np.zeros(3, dtype=capi.PRIOR_CALL_DTYPE)
        assert e._L.dmx_engine_get_prior_calls(e._h, out.ctypes.data) == capi.DMX_ERR_STATE
        assert e._L.dmx_engine_get_prior_fit(e._h, *([None] * 11), 0) == capi.DMX_ERR_STATE
        assert code(e.prior_step, pi, 0.1) == capi.DMX_ERR_STATE            # no doublet grid yet and grid == NULL
        assert code(e.prior_fit) == capi.DMX_ERR_STATE
        assert code(e.prior_call, pi, 0.1) == capi.DMX_ERR_STATE
        for bad_pi in (np.array([0.5, np.nan, 0.25, 0.25]), np.array([0.5, -0.1, 0.3, 0.3]), np.zeros(V), np.array([0.5, np.inf, 0.1, 0.1])):
            assert code(e.prior_step, bad_pi, 0.1, grid=grid) == capi.DMX_ERR_ARG
            assert code(e.prior_call, bad_pi, 0.1, grid=grid) == capi.DMX_ERR_ARG
            assert code(e.prior_fit, grid=grid, pi0=bad_pi) == capi.DMX_ERR_ARG
        for bad_d in (-0.01, 1.01, np.nan):
            assert code(e.prior_step, pi, bad_d, grid=grid) == capi.DMX_ERR_ARG
            assert code(e.prior_fit, grid=grid, d0=bad_d) == capi.DMX_ERR_ARG
        assert code(e.prior_step, pi, 0.1, grid=grid, mask=np.zeros(3)) == capi.DMX_ERR_ARG      # B_in == 0
        assert code(e.prior_fit, grid=grid, mask=np.zeros(3)) == capi.DMX_ERR_ARG
        assert code(e.prior_step, pi, 0.1, grid=np.full((3, V, V, 2), -np.inf)) == capi.DMX_ERR_ARG
        assert code(e.prior_fit, grid=grid, max_iter=0) == capi.DMX_ERR_ARG
        for field, val in (("n_samples", V + 1), ("n_alpha", 3), ("n_cells", 0), ("n_cells", -1), ("grid_memory", 7)):
            rq, keep = e._prior_request(grid, None)
            setattr(rq, field, val)
            assert e._L.dmx_engine_prior_step(e._h, C.byref(rq), pi.ctypes.data, 0.1) == capi.DMX_ERR_ARG, field
        rq, keep = e._prior_request(grid, None)
        assert e._L.dmx_engine_prior_step(e._h, C.byref(rq), None, 0.1) == capi.DMX_ERR_ARG
        s = e.prior_step(pi, 0.1, grid=grid)          # and the engine still works
        assert s["b_in"] == 3
    finally:
        e.close()
    # sizes: n_cells against the staged pileup; one alpha; V A beyond the limit (checked before the grid is looked at)
    es = staged["e"]
    rq, keep = es._prior_request(None, None)
    rq.n_cells = staged["B"] - 1
    assert es._L.dmx_engine_prior_step(es._h, C.byref(rq), np.full(8, 0.125).ctypes.data, 0.1) == capi.DMX_ERR_ARG
    e1 = eng.Engine(V, (0.0,))
    try:
        rq = capi.PriorRequest(3, V, 1, capi.DMX_MEM_HOST, grid.ctypes.data, None)
        assert e1._L.dmx_engine_prior_step(e1._h, C.byref(rq), pi.ctypes.data, 0.1) == capi.DMX_ERR_ARG
    finally:
        e1.close()
    e2 = eng.Engine(2049, (0.0, 0.5))
    try:
        p2 = np.full(2049, 1.0 / 2049)
        rq = capi.PriorRequest(1, 2049, 2, capi.DMX_MEM_HOST, grid.ctypes.data, None)
        assert e2._L.dmx_engine_prior_step(e2._h, C.byref(rq), p2.ctypes.data, 0.1) == capi.DMX_ERR_ARG
        assert b"4096" in e2._L.dmx_last_error()
    finally:
        e2.close()


def test_a_request_that_cannot_fit_is_refused_before_anything_is_allocated(m):
    """n_cells so large that the buffers exceed the free memory, over a small real grid: the need is added up and compared with the free
    memory before the grid is read or anything is allocated, so the call returns DMX_ERR_NOMEM at once.  A host grid (its device copy
    alone would be 550 GB) for step, fit and call, and a device grid on a 2 048-donor engine (35 TB of rows) for step and fit.  The earlier step's, fit's
    and call's results are still readable, and a small call afterwards is right."""
    import ctypes as C
    capi = m["capi"]
    V, A, B = 4, 2, 30
    rng = np.random.default_rng(9)
    grid = random_grid(rng, B, V, A)
    pi, d = random_pi(rng, V, False), 0.2
    tg = m["torch"].from_numpy(grid).cuda()
    m["torch"].cuda.synchronize()
    e = m["engine"].Engine(V, ALPHAS[A])
    try:
        first = e.prior_step(pi, d, grid=grid, rows=True)
        fit = e.prior_fit(grid=grid, max_iter=3, tol=0.0)
        first = e.prior_step(pi, d, grid=grid, rows=True)          # (the fit overwrote the first step's rows)
        calls = e.prior_call(pi, d, grid=grid)
        info = e.prior_info()
        total = m["torch"].cuda.mem_get_info(0)[1]
        huge = 2 ** 31 - 1

        def refused(eng, Vx, mem, ptr, pix, fns, need):
            assert need > total                      # (more than the whole card, free or not: nothing below may go on to run)
            for fn in fns:
                rq = capi.PriorRequest(huge, Vx, A, mem, ptr, None)
                rq.d0, rq.tol, rq.max_iter = 0.1, 0.0, 3
                if fn == "fit":
                    rc = eng._L.dmx_engine_prior_fit(eng._h, C.byref(rq))
                else:
                    rc = getattr(eng._L, f"dmx_engine_prior_{fn}")(eng._h, C.byref(rq), pix.ctypes.data, d)
                msg = eng._L.dmx_last_error().decode()
                assert rc == capi.DMX_ERR_NOMEM, (mem, fn, rc, msg)
                assert f"dmx_engine_prior_{fn}" in msg and "device bytes" in msg and "are free" in msg and str(huge) in msg
        # a host grid: its device copy alone is 8 (2^31 - 1) V V A bytes = 550 GB
        refused(e, V, capi.DMX_MEM_HOST, grid.ctypes.data, pi, ("step", "fit", "call"), 8 * huge * V * V * A)
        # a device grid on a 2 048-donor engine: the rows are 8 (2^31 - 1) (V + 3) bytes = 35 TB (the records alone, 172 GB, could fit)
        e2 = m["engine"].Engine(2048, ALPHAS[A])
        try:
            refused(e2, 2048, capi.DMX_MEM_DEVICE, int(tg.data_ptr()), np.full(2048, 1.0 / 2048), ("step", "fit"), 8 * huge * 2051)
        finally:
            e2.close()
        # the refused calls touched nothing
        kept = e.get_prior_step(rows=True)
        for k in ("N", "pi_next", "rows", "flags"):
            assert kept[k].tobytes() == first[k].tobytes(), k
        assert (kept["ll"], kept["hom"], kept["het"], kept["b_in"], kept["d_next"]) == (first["ll"], first["hom"], first["het"], first["b_in"], first["d_next"])
        again = np.zeros(B, dtype=capi.PRIOR_CALL_DTYPE)
        capi.check(e._L.dmx_engine_get_prior_calls(e._h, again.ctypes.data))
        assert again.tobytes() == calls.tobytes()
        pi2 = np.zeros(V); d2 = C.c_double(); n2 = C.c_int32()
        capi.check(e._L.dmx_engine_get_prior_fit(e._h, pi2.ctypes.data, C.byref(d2), None, C.byref(n2), *([None] * 7), 0))
        assert pi2.tobytes() == fit["pi"].tobytes() and d2.value == fit["d"] and n2.value == 3
        assert e.prior_info()["n_cells"] == info["n_cells"]
        # and a small call afterwards is right
        small = e.prior_step(pi, d, grid=grid[:7], rows=True)
        assert small["rows"].tobytes() == first["rows"][:7].tobytes()
        check_step(small, R.step(grid[:7], pi, d), V)
    finally:
        e.close()


def test_largest_panel(m):
    """V A = 4096 (V = 2048, A = 2), the limit: one wavefront per workgroup and 96 KiB of LDS.  One barcode with a handful of finite
    entries (the rest -inf), so the restatement stays small."""
    V, A = 2048, 2
    grid = np.full((2, V, V, A), -np.inf)
    rng = np.random.default_rng(8)
    js = rng.integers(0, V, size=40); ks = (js + 1 + rng.integers(0, V - 1, size=40)) % V
    grid[0, js, ks, 1] = -10.0 * rng.random(40)
    grid[0, js[:5], 0, 0] = -3.0 * rng.random(5)
    grid[0, V - 1, V - 2, 1] = -0.5
    grid[1, 7, 0, 0] = -2.0
    pi = random_pi(rng, V, False)
    e = m["engine"].Engine(V, ALPHAS[A])
    try:
        s = e.prior_step(pi, 0.3, grid=grid, rows=True)
        assert e.prior_info()["waves_per_block"] == 1
        check_step(s, R.step(grid, pi, 0.3), V)
    finally:
        e.close()


@pytest.mark.parametrize("fast", [False, True])
def test_end_to_end(m, oracle, tmp_path, fast):
    eng, prior, capi = m["engine"], m["prior"], m["capi"]
    sp, truth, g = P.make(m["synth"], eng.geno_from_gt)
    pl = host_pileup(m, sp)
    sms = [f"s{j}" for j in range(P.V)]
    bcs = [m["synth"].barcode_name(i) for i in range(sp.n_cells)]
    mode = capi.DMX_MODE_FAST if fast else capi.DMX_MODE_STRICT
    r = prior.prior_run(pl, g, sms, str(tmp_path / "p"), alphas=P.ALPHAS, barcodes=bcs, mode=mode)
    eng.demuxlet_run(pl, g, sms, P.ALPHAS, str(tmp_path / "plain"), barcodes=bcs, mode=mode)
    assert (tmp_path / "p.best").read_bytes() == (tmp_path / "plain.best").read_bytes()
    for ext in ("single", "sing2"):
        assert (tmp_path / f"p.{ext}").read_bytes() == (tmp_path / f"plain.{ext}").read_bytes()
    f = r["fit"]
    print("end to end:", "fast" if fast else "strict", f["n_iter"], f["converged"], f["pi"], truth["cell_share"], f["d"], truth["doublet_rate"])
    assert f["converged"]
    assert f["pi"][P.ABSENT] < P.CAP_ABSENT
    assert np.abs(f["pi"] - truth["cell_share"]).max() < P.CAP_SHARE
    assert abs(f["d"] - truth["doublet_rate"]) < P.CAP_RATE
    # the device grid against the oracle's
    e = eng.Engine(P.V, P.ALPHAS, mode=mode)
    try:
        e.set_genotypes(g); e.set_pileup(pl); e.run_doublet()
        dev = e.get_doublet()[0]
    finally:
        e.close()
    ref = P.oracle_grid(oracle, sp, g)
    used = np.zeros((P.V, P.V, len(P.ALPHAS)), dtype=bool)
    used[:, 0, 0] = True
    used[:, :, 1:] = ~np.eye(P.V, dtype=bool)[:, :, None]
    assert (np.abs(dev[:, used] - ref[:, used]) <= 1e-9 * np.maximum(1.0, np.abs(ref[:, used]))).all()
    # the files
    lines = (tmp_path / "p.prior.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["SM_ID", "SHARE", "N.CELL"] and [x.split("\t")[0] for x in lines[1:1 + P.V]] == sms
    trailer = dict(x[1:].split("\t") for x in lines[1 + P.V:])
    assert list(trailer) == ["RATE.DBL", "RATE.HET", "N.HOM", "N.BARCODE", "LLK", "ITER", "CONVERGED"]
    assert abs(float(trailer["RATE.DBL"]) - f["d"]) < 1e-6 and int(trailer["ITER"]) == f["n_iter"] and trailer["CONVERGED"] == "1"
    assert abs(float(trailer["RATE.HET"]) - f["d"] * (1 - float(np.sum(f["pi"] ** 2)))) < 1e-6
    fit_lines = (tmp_path / "p.prior_fit.tsv").read_text().splitlines()
    assert fit_lines[0].split("\t") == ["ITER", "LLK", "RATE.DBL"] and len(fit_lines) == 1 + f["n_iter"]
    eb = [x.split("\t") for x in (tmp_path / "p.eb.tsv").read_text().splitlines()]
    assert eb[0] == ["BARCODE", "N.SNP", "BEST", "CALL", "PRB.SNG", "PRB.HET", "PRB.HOM", "SNG.1ST", "PRB.SNG1", "SNG.2ND", "PRB.SNG2", "DBL.1ST",
                     "DBL.2ND", "ALPHA", "PRB.DBL1", "LLK.EVID"]
    best = [x.split("\t") for x in (tmp_path / "p.best").read_text().splitlines()]
    bcol = best[0].index("BARCODE"); kcol = best[0].index("BEST")
    assert [x[0] for x in eb[1:]] == [x[bcol] for x in best[1:]] and [x[2] for x in eb[1:]] == [x[kcol] for x in best[1:]]
    for x in eb[1:]:
        assert abs(float(x[4]) + float(x[5]) + float(x[6]) - 1.0) < 1e-4
        kind = x[3].split("-")[0]
        assert kind in ("SNG", "DBL", "AMB")
        if x[11] != "." and x[13] == "0.500":
            assert sms.index(x[11]) < sms.index(x[12])
        if kind == "DBL":
            assert (x[11], x[12]) == tuple(x[3].split("-")[1:3])
            assert float(x[5]) >= 0.9 and sms.index(x[3].split("-")[1]) < sms.index(x[3].split("-")[2]) and x[3].endswith("-0.500")
        elif kind == "SNG":
            assert float(x[8]) >= 0.9 and x[3] == "SNG-" + x[7]
    # right calls against truth, for the record (no bound: the quality table is tools/bench_prior.py's)
    order = r["order"]
    call_ok = best_ok = 0
    for row, k in zip(eb[1:], order):
        a, b = int(truth["first"][k]), int(truth["second"][k])
        het = b >= 0 and b != a
        want = ("DBL", {sms[a], sms[b]}) if het else ("SNG", {sms[a]})
        for col, tally in ((3, "call"), (2, "best")):
            t = row[col].split("-")
            got = (t[0], set(t[1:3]) if t[0] == "DBL" else {t[1]})
            if got == want:
                if tally == "call":
                    call_ok += 1
                else:
                    best_ok += 1
    print("right calls: CALL", call_ok / len(order), "BEST", best_ok / len(order))
