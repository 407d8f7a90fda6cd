"""CPU: the crafted `.pair` barcodes of pair_craft.py are what they claim to be, and the host formatter prints a certified barcode from the grid WITH its
certified entries — the reference the device text is compared with (test_gpu_pair_text.py).

For every case (V = 4 and 7; alphas (0, 0.5) and (0, 0.25, 0.5); delta = 5e-12 and 5e-11, both signs; a singlet and a doublet probe row):
  * mpmath: the probe's true scaled posterior is >= 1e-12 from a rounding boundary on one side with the certified entries and >= 1e-12 on the other side
    without them; every other row is >= 1e-9 from every boundary;
  * '%.5g' of the host chain (the expression of cmd_cram_demuxlet.cpp:780 / :792 on call_cell's scalars) differs between the two on the probe row;
  * dmx_write_doublet on the substituted grid prints the certified digits (dmx_host.cpp: the scratch grid of a certified barcode goes through call_cell);
  * every other row prints the same bytes from either set of scalars."""
import math

import numpy as np
import pytest

import pair_craft as pc

CONFIGS = [(4, (0.0, 0.5)), (7, (0.0, 0.25, 0.5)), (4, (0.0, 0.25, 0.5)), (7, (0.0, 0.5))]


@pytest.fixture(scope="module")
def eng():
    from demuxlet_amd import build, engine
    build.build()
    return engine


def test_k3_scalars_is_call_cells_expression():
    rng = np.random.default_rng(1)
    V, alphas = 5, (0.0, 0.25, 0.5)
    g = -rng.uniform(0, 40, size=(V, V, 3))
    mx, ss, sd = pc.k3_scalars(g, alphas)
    assert mx == g.max()
    w = pc._weights(V, alphas, 0.5)
    tot = float(np.sum(w * np.exp(g - mx)))
    assert abs(ss + sd - tot) <= 1e-14 * tot
    assert abs(ss - float(np.sum(np.exp(g[:, 0, 0] - mx)) * 0.5 / V)) <= 1e-14 * ss
    g[3, 1, 2] = math.nan                                     # the maximum skips NaN (fmax); the sum does not
    mx2, ss2, sd2 = pc.k3_scalars(g, alphas)
    assert mx2 == np.nanmax(g) and ss2 == ss and math.isnan(sd2)
    g[3, 1, 2] = -1.0
    g[2, 2, 1] = math.inf                                     # an entry that is never printed and never summed still is the maximum
    assert pc.k3_scalars(g, alphas) == (math.inf, 0.0, 0.0)


@pytest.mark.parametrize("V,alphas", CONFIGS)
def test_straddle_cases_are_what_they_claim(eng, tmp_path, V, alphas):
    cases = pc.straddle_cases(V, alphas)
    assert len(cases) == 8 and {(c.delta, c.sign, c.probe[2] == 0) for c in cases} == {(d, s, k) for d in (5e-12, 5e-11) for s in (1, -1) for k in (True, False)}
    A = len(alphas)
    rows = pc.rows_of(V, alphas)
    grids = np.stack([pc.substituted(c.grid, c.ovr) for c in cases])
    B = len(cases)
    bcs = [f"BC{i:03d}-1" for i in range(B)]
    sms = [f"SM{j}" for j in range(V)]
    ones = np.ones(B, dtype=np.int32)
    fa = eng.FinalArgs(bcs, sms, alphas, pc.PRIOR, ones, ones, ones, ones, write_pair=True)
    eng.write_doublet(fa, grids, np.zeros((B, A)), str(tmp_path / "h"))
    lines = (tmp_path / "h.pair").read_bytes().split(b"\n")[1:-1]
    assert len(lines) == B * len(rows)
    for i, c in enumerate(cases):
        a, b, n, v_ab, v_ba = c.ovr
        assert alphas[n] == 0.5 and a < b and v_ab == v_ba == c.grid[a, b, n] + c.sign * c.delta
        dc, du, other = pc.check_case(c)
        assert abs(dc) >= pc.PROBE_MARGIN and abs(du) >= pc.PROBE_MARGIN and dc * du < 0, (i, dc, du)
        assert other >= pc.OTHER_MARGIN, (i, other)
        gs = grids[i]
        su, sc = pc.k3_scalars(c.grid, alphas), pc.k3_scalars(gs, alphas)
        assert (su[1] + su[2]) * 0.9 < pc.PRIOR / V / (V - 1) / (A - 1) / 2.0 * (1.0 + math.exp(c.grid[b, a, n] - su[0]))   # the best doublet holds most of the posterior
        assert all(-600.0 <= v - sc[0] <= 0.0 for v in gs.reshape(-1))
        for r, ln in zip(rows, lines[i * len(rows):(i + 1) * len(rows)]):
            v = float(gs[pc.entry_of(r)])
            f = ln.split(b"\t")
            want_c = ("%.5g" % pc.host_post(v, sc, V, A, r[2] == 0)).encode()
            want_u = ("%.5g" % pc.host_post(v, su, V, A, r[2] == 0)).encode()
            assert f[0] == bcs[i].encode() and f[4] == ("%.5f" % v).encode()
            assert f[5] == want_c, (i, r, f[5], want_c)
            assert (want_c != want_u) == (r == c.probe), (i, r, want_c, want_u)
