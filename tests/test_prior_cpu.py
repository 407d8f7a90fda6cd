"""CPU: the empirical-Bayes prior model in its numpy restatement (tests/prior_ref.py), the recovery of a
make_pool_pileup pool's shares and doublet rate from the CPU oracle's grids, and the binding's struct layouts.  No GPU compute."""
import ctypes as C
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import prior_pool as P
import prior_ref as R

ROOT = Path(__file__).resolve().parents[1]


def random_grid(rng, B, V, A, scale=30.0):
    return -scale * rng.random((B, V, V, A))


def test_weights_sum_to_one():
    rng = np.random.default_rng(1)
    for V in (2, 3, 7, 33):
        for A in (2, 3, 5):
            for d in (0.0, 0.3, 1.0):
                pi = rng.random(V)
                pi[rng.random(V) < 0.3] = 0.0
                pi[0] = max(pi[0], 0.1)
                p, wS, wD = R.weights(pi, d, A)
                assert abs(p.sum() - 1.0) < 1e-14
                assert (wD[np.diag_indices(V)] == 0).all()
                assert abs(wS.sum() + (A - 1) * wD.sum() - 1.0) < 1e-13
                assert (wS[p == 0] == 0).all() and (wD[p == 0] == 0).all() and (wD[:, p == 0] == 0).all()
    # prior.uniform_rate: with uniform shares the doublet and singlet-like weights stand as the reference's p / 2 to 1 - p
    # (cmd_cram_demuxlet.cpp:726-731 on a grid whose alphas above 0 are 0.5: both orders of a pair, each at half weight)
    from demuxlet_amd import prior
    for V in (2, 8, 33):
        for p in (0.1, 0.5, 0.9):
            _, wS, wD = R.weights(np.full(V, 1.0 / V), prior.uniform_rate(p, V), 2)
            assert abs(wD.sum() / wS.sum() - (p / 2) / (1 - p)) < 1e-12 * (p / 2) / (1 - p) + 1e-15
    assert prior.uniform_rate(1.0, 5) == 1.0 and prior.uniform_rate(0.0, 5) == 0.0


def test_ll_never_decreases():
    rng = np.random.default_rng(2)
    for V, A, B in ((3, 2, 40), (5, 3, 30), (8, 2, 25)):
        grid = random_grid(rng, B, V, A)
        pi, d = np.full(V, 1.0 / V), 0.5
        prev = -np.inf
        for it in range(50):
            s = R.step(grid, pi, d)
            assert s["ll"] >= prev - 1e-9 * max(1.0, abs(s["ll"])), (V, A, it)
            prev = s["ll"]
            pi, d = s["pi_next"], s["d_next"]


def test_exact_zeros_stay_exact():
    rng = np.random.default_rng(3)
    V, A, B = 6, 3, 50
    grid = random_grid(rng, B, V, A)
    grid[:, 2] += 40.0                              # the evidence favours the donor that the prior rules out
    pi = np.array([0.3, 0.2, 0.0, 0.5, 0.0, 0.1])
    d = 0.3
    for it in range(5):
        s = R.step(grid, pi, d)
        assert s["N"][2] == 0.0 and s["N"][4] == 0.0
        assert s["pi_next"][2] == 0.0 and s["pi_next"][4] == 0.0
        pi, d = s["pi_next"], s["d_next"]
    s0 = R.step(grid, pi, 0.0)                       # d = 0: no doublet mass at all
    assert s0["het"] == 0.0 and s0["hom"] == 0.0 and s0["d_next"] == 0.0
    s1 = R.step(grid, pi, 1.0)                       # d = 1: every singlet-like term is a homotypic doublet
    assert abs(s1["hom"] + s1["het"] - s1["b_in"]) < 1e-9


def test_flags_and_records():
    rng = np.random.default_rng(4)
    V, A, B = 4, 2, 6
    grid = random_grid(rng, B, V, A)
    grid[1, 2, 1, 1] = np.nan                        # a used entry
    grid[2, 1, 1, 1] = np.nan                        # the diagonal: not used
    grid[2, 1, 2, 0] = np.nan                        # [j][k != 0][0]: not used
    grid[3] = -np.inf
    mask = np.array([1, 1, 1, 1, 0, 1])
    s = R.step(grid, np.full(V, 0.25), 0.2, mask)
    from demuxlet_amd import capi, prior
    assert (R.MASKED, R.BAD) == (capi.DMX_PRIOR_MASKED, capi.DMX_PRIOR_BAD)          # the restatement's flags are the header's
    assert list(s["flags"]) == [0, R.BAD, 0, R.BAD, R.MASKED, 0] and s["b_in"] == 3
    assert (s["rows"][[1, 3, 4]] == 0).all()
    assert np.array_equal(R.fold_chunked(s["rows"], s["flags"])[:V], s["rows"][[0, 2, 5]][:, :V].sum(axis=0))
    c = R.call(grid, np.full(V, 0.25), 0.2, mask)
    ok = c["flag"] == 0
    assert np.allclose((c["p_sng"] + c["p_het"] + c["p_hom"])[ok], 1.0, atol=1e-12)
    assert (c["i_sng1"][~ok] == -1).all() and (c["p_het"][~ok] == 0).all()
    dup = random_grid(rng, 1, V, A)
    dup[0, :, 0, 0] = -5.0                           # every singlet ties: the first two win
    dup[0, :, :, 1] = -7.0                           # every doublet ties: (0, 1, 1) wins
    c = R.call(dup, np.full(V, 0.25), 0.2)
    assert (c["i_sng1"][0], c["i_sng2"][0], c["j_dbl"][0], c["k_dbl"][0], c["n_dbl"][0]) == (0, 1, 0, 1, 1)
    # the front end's spelling of a record: DBL.1ST / DBL.2ND and CALL in one order, a before b at alpha = 0.5 only
    sms = ["s0", "s1", "s2", "s3"]
    rec = dict(j_dbl=3, k_dbl=1, n_dbl=1, p_het=0.95, p_sng1=0.04, i_sng1=3, i_sng2=1)
    assert prior.dbl_pair(rec, (0.0, 0.5)) == (1, 3, 0.5) and prior.eb_call(rec, (0.0, 0.5), sms, 0.9) == "DBL-s1-s3-0.500"
    assert prior.dbl_pair(rec, (0.0, 0.25)) == (3, 1, 0.25) and prior.eb_call(rec, (0.0, 0.25), sms, 0.9) == "DBL-s3-s1-0.250"
    rec.update(p_het=0.5, p_sng1=0.45)
    assert prior.eb_call(rec, (0.0, 0.5), sms, 0.9) == "AMB-s3-s1-s1/s3"
    rec.update(p_het=0.02, p_sng1=0.97)
    assert prior.eb_call(rec, (0.0, 0.5), sms, 0.9) == "SNG-s3"
    none = dict(j_dbl=-1, k_dbl=-1, n_dbl=-1, p_het=0.0, p_sng1=1.0, i_sng1=2, i_sng2=0)
    assert prior.dbl_pair(none, (0.0, 0.5)) == (-1, -1, 0.0) and prior.eb_call(none, (0.0, 0.5), sms, 0.9) == "SNG-s2"


def test_recovery_on_the_oracle_grids(oracle):
    """The restatement alone on the CPU oracle's grids of the shared pool (tests/prior_pool.py).  Achieved with this seed: absent donor
    share below 5e-5 (prints as 0.0000), largest share error 0.003, d = 0.186 against a drawn rate of 0.202 (0.016 apart), converged
    after 7 iterations at tol 1e-6.  The caps below are conditions, not these values."""
    from demuxlet_amd import synth
    sp, truth, g = P.make(synth, oracle.geno_from_gt)
    grid = P.oracle_grid(oracle, sp, g)
    mask = np.diff(sp.cell_pair_off) > 0
    f = R.fit(grid, None, 0.1, 200, 1e-6, mask)
    print("prior recovery:", f["n_iter"], f["converged"], np.round(np.asarray(f["pi"], dtype=float), 4), truth["cell_share"], float(f["d"]),
          truth["doublet_rate"])
    assert f["converged"] and f["n_iter"] < 200
    assert f["pi"][P.ABSENT] < P.CAP_ABSENT
    assert np.abs(f["pi"] - truth["cell_share"]).max() < P.CAP_SHARE
    assert abs(f["d"] - truth["doublet_rate"]) < P.CAP_RATE
    assert (np.diff(f["ll_trace"]) >= -1e-9 * np.abs(f["ll_trace"][1:])).all()


def test_make_pool_pileup_truth():
    from demuxlet_amd import synth
    rng = np.random.default_rng(5)
    raw = synth.make_raw_genotypes(rng, 50, 4)
    sp, t = synth.make_pool_pileup(rng, raw.alleles, 4000, 0.1, 1.5, (0.5, 0.3, 0.2, 0.0), 0.25)
    assert sp.n_cells == 4000 and sp.truth.shape == (4000, 2)
    assert (t["first"] != 3).all() and (t["second"] != 3).all()
    assert ((t["second"] >= 0) == t["doublet"]).all()
    assert t["homotypic"].sum() > 0 and (t["second"][t["homotypic"]] == t["first"][t["homotypic"]]).all()
    assert abs(t["doublet_rate"] - 0.25) < 0.03 and np.abs(t["cell_share"] - np.array([0.5, 0.3, 0.2, 0.0])).max() < 0.03
    hom_expected = 0.25 * (0.25 + 0.09 + 0.04)
    assert abs(t["homotypic"].mean() - hom_expected) < 0.02


def test_struct_sizes_match_the_header():
    """dmx_prior_request / dmx_prior_call / dmx_prior_info: the binding's sizes and a late member's offset against the C compiler's."""
    from demuxlet_amd import capi
    src = ('#include "dmx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", '
           'sizeof(dmx_prior_request), offsetof(dmx_prior_request, fix_d), sizeof(dmx_prior_call), offsetof(dmx_prior_call, flag), '
           'sizeof(dmx_prior_info), offsetof(dmx_prior_info, waves_per_block));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        got = list(map(int, subprocess.check_output([str(Path(d) / "s")], text=True).split()))
    assert got == [C.sizeof(capi.PriorRequest), capi.PriorRequest.fix_d.offset, C.sizeof(capi.PriorCall), capi.PriorCall.flag.offset,
                   C.sizeof(capi.PriorInfo), capi.PriorInfo.waves_per_block.offset]
    assert capi.PRIOR_CALL_DTYPE.itemsize == C.sizeof(capi.PriorCall)
    assert [capi.PRIOR_CALL_DTYPE.fields[n][1] for n, _ in capi.PriorCall._fields_] == [getattr(capi.PriorCall, n).offset for n, _ in capi.PriorCall._fields_]


def test_entry_points_are_bound():
    from demuxlet_amd import capi, engine
    for name in ("dmx_engine_prior_step", "dmx_engine_get_prior_step", "dmx_engine_prior_fit", "dmx_engine_get_prior_fit",
                 "dmx_engine_prior_call", "dmx_engine_get_prior_calls", "dmx_engine_prior_info"):
        assert name in capi.SYMBOLS
    for name in ("prior_step", "prior_fit", "prior_call", "prior_info"):
        assert callable(getattr(engine.Engine, name))
