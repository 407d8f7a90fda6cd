"""CPU: the restatement of the continuous mixing share (tests/share_ref.py) and the host side of demuxlet_amd/share.py.

LL' and LL'' against central finite differences of the restated LL; LL'' < 0 for one-hot rows; LL at rho = 0 against the existing
restatement of the ambient-aware doublet profile; every branch of the restated driver; the candidate selection (ties, one unordered pair
once, the plain pass's pair always there); the decision rule, both writers and the command line's errors."""
import numpy as np
import pytest

import ambient_dbl_ref as D
import share_ref as R

LD = np.longdouble


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import capi, engine, share, synth
    return dict(capi=capi, engine=engine, share=share, synth=synth)


@pytest.fixture(scope="module")
def prob(m):
    rng = np.random.default_rng(2801)
    S, V, B = 120, 4, 6
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = np.stack([m["engine"].geno_from_gp(x, 0.01) for x in m["synth"].raw_gp_from_alleles(rng, raw.alleles)])
    sp, rho, alpha, a = m["synth"].make_ambient_mixed_pileup(rng, raw.alleles, B, 0.5, 2.5, 0.1, np.arange(B) % 2 == 0, 0.25)
    hot = np.zeros_like(g)
    dos = np.clip(raw.alleles, 0, 1).sum(axis=2)
    for k in range(3):
        hot[:, :, k] = dos == k
    mat, err = m["engine"].phred_tables()
    return dict(sp=sp, g=g, hot=hot, a=a, rho=rho, mat=mat, err=err, B=B, V=V, S=S, truth=sp.truth)


@pytest.mark.parametrize("with_rho", [False, True])
def test_derivatives_against_finite_differences(prob, with_rho):
    ref = R.ShareRef(prob["sp"], prob["g"], prob["mat"], prob["err"], prob["a"] if with_rho else None, np.full(prob["B"], 0.2) if with_rho else None)
    h = 1e-6                                          # long double: the differences' rounding stays below 1e-4 of LL''
    for b in range(prob["B"]):
        for al in (0.01, 0.3, 0.5, 0.99):
            e0, ep, em = (ref.evaluate(b, 0, 1, x) for x in (al, al + h, al - h))
            fd1 = (ep.ll - em.ll) / (2 * h)
            fd2 = (ep.ll - 2 * e0.ll + em.ll) / (h * h)
            assert abs(float(fd1 - e0.d1)) <= 1e-6 * max(1.0, e0.m1), (b, al, float(fd1), float(e0.d1))
            assert abs(float(fd2 - e0.d2)) <= 1e-4 * max(1.0, e0.m2), (b, al, float(fd2), float(e0.d2))


def test_one_hot_rows_are_concave(prob):
    ref = R.ShareRef(prob["sp"], prob["hot"], prob["mat"], prob["err"])
    n = 0
    for b in range(prob["B"]):
        for v1, v2 in ((0, 1), (2, 3), (3, 0)):
            for al in np.linspace(0.0, 1.0, 11):
                e = ref.evaluate(b, v1, v2, float(al))
                if np.isfinite(float(e.ll)):
                    assert e.d2 < 0, (b, v1, v2, al, float(e.d2))
                    n += 1
    assert n > 50


def test_ll_is_the_ambient_doublet_restatement(prob):
    sp = prob["sp"]
    ref = R.ShareRef(sp, prob["g"], prob["mat"], prob["err"])
    cand = np.tile(np.array([[[0, 1], [2, 1]]], dtype=np.int32), (prob["B"], 1, 1))
    alphas = np.array([0.0, 0.2, 0.5, 1.0])
    LL, ns, nr = D.ref_dbl_profile(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, cand, prob["g"], np.zeros(prob["S"]), alphas, np.array([0.0]),
                                   prob["mat"], prob["err"])
    for b in range(prob["B"]):
        for c in range(2):
            for i, al in enumerate(alphas):
                e = ref.evaluate(b, int(cand[b, c, 0]), int(cand[b, c, 1]), float(al))
                assert abs(float(e.ll) - LL[b, c, i, 0]) <= 1e-9
                assert (e.n_snp, e.n_read) == (ns[b, c], nr[b, c])


def quad(peak, curv=-50.0, off=-100.0):
    return lambda a: (off + 0.5 * curv * (a - peak) ** 2, curv * (a - peak), curv)


def test_driver_branches(prob):
    smooth = lambda a: (30.0 * np.log(0.1 + a) - 60.0 * a, 30.0 / (0.1 + a) - 60.0, -30.0 / (0.1 + a) ** 2)      # maximum at 0.4
    r = R.driver(smooth)
    assert r["status"] == R.INTERIOR and abs(r["alpha"] - 0.4) <= 1e-6 and 5 <= r["n_eval"] <= 9   # 0, 1, start, Newton steps, final
    r = R.driver(quad(-0.2))
    assert r["status"] == R.AT_0 and r["alpha"] == 0.0 and r["n_eval"] == 2 and r["at"] == r["at0"]
    r = R.driver(quad(1.2))
    assert r["status"] == R.AT_1 and r["alpha"] == 1.0 and r["n_eval"] == 2 and r["at"] == r["at1"]
    r = R.driver(quad(0.4, curv=50.0))                      # convex: both ends are local maxima, the larger LL is at 1
    assert r["status"] == (R.AT_1 | R.FLAT) and r["alpha"] == 1.0
    r = R.driver(quad(0.5, curv=50.0))                      # a tie goes to 0
    assert r["status"] == (R.AT_0 | R.FLAT) and r["alpha"] == 0.0
    cubic = lambda a: (-(a - 0.2) ** 4, -4 * (a - 0.2) ** 3, -12 * (a - 0.2) ** 2)     # Newton converges linearly here
    r = R.driver(cubic, max_iter=3)
    assert r["status"] == (R.INTERIOR | R.NOT_CONVERGED) and r["n_eval"] == 2 + 3 + 1
    r = R.driver(cubic, max_iter=200, tol=1e-9)
    assert r["status"] == R.INTERIOR and abs(r["alpha"] - 0.2) <= 1e-8
    r = R.driver(lambda a: (float("-inf"), float("nan"), float("nan")))
    assert r["status"] == (R.AT_0 | R.NONFINITE) and r["n_eval"] == 2
    # Newton steps that leave the bracket are replaced by its midpoint
    steep = lambda a: (0.0, 1.0 - 2.0 * (a > 0.1), -1e-3)
    near = []
    r = R.driver(steep, tol=1e-3, near=near)
    assert r["status"] & R.INTERIOR and abs(r["alpha"] - 0.1) <= 2e-3 and near


def test_driver_flat_profile_of_identical_rows(prob):
    g = prob["hot"].copy()
    g[:, 1] = g[:, 0]
    ref = R.ShareRef(prob["sp"], g, prob["mat"], prob["err"])
    r = R.driver(lambda a: ref.evaluate(1, 0, 1, a).values())
    assert r["status"] == (R.AT_0 | R.FLAT) and r["alpha"] == 0.0 and r["at"][1] == 0.0 and r["at"][2] == 0.0


def test_driver_on_a_doublet_finds_the_reference_maximum(prob):
    ref = R.ShareRef(prob["sp"], prob["hot"], prob["mat"], prob["err"])
    b = 0
    v1, v2 = (int(x) for x in prob["truth"][b])
    r = R.driver(lambda a: ref.evaluate(b, v1, v2, a).values())
    assert r["status"] == R.INTERIOR
    a_star, e_star = R.maximise(lambda a: ref.evaluate(b, v1, v2, a))
    assert abs(r["alpha"] - a_star) <= 2e-6 and r["at"][0] >= float(e_star.ll) - 1e-9
    assert 0.05 < a_star < 0.6


def test_anchors_and_candidate_selection(m):
    sh = m["share"]
    llks = np.array([[-5.0, -1.0, -1.0, -9.0], [-2.0, -3.0, -4.0, -1.0]])
    assert sh.anchors_from_singlet(llks, 2).tolist() == [[1, 2], [3, 0]]                     # the first maximum in ascending order
    assert sh.anchors_from_singlet(llks[:, :1], 2).tolist() == [[0, -1], [0, -1]]
    B, T, V = 2, 2, 5
    scan = np.zeros((B, T, V, 3))
    scan[..., 2] = -4.0                                                                      # z = d1 / 2
    anchors = np.array([[0, 1], [2, -1]], dtype=np.int32)
    scan[0, 0, :, 1] = [0.0, 6.0, 6.0, 2.0, -1.0]      # anchor 0: partners 1 and 2 tie, 3 lower, 4 has LL' < 0
    scan[0, 1, :, 1] = [8.0, 0.0, 6.0, 0.0, 3.0]       # anchor 1: partner 0 is the pair (0, 1) again, with the higher z
    scan[1, 0, :, 1] = [1.0, 2.0, 0.0, 3.0, 4.0]
    scan[1, 0, 4, 2] = 1.0                             # LL'' > 0: not ranked
    scan[1, 1, :, 1] = 50.0                            # an unused anchor slot is never read
    cand, pick = sh.select_candidates(scan, anchors, 3, np.array([3, 2]), np.array([4, 3]))
    assert cand[0].tolist() == [[1, 0], [0, 2], [1, 2], [3, 4]]                              # z 4, then the tie at 3 by (t, v); (0, 1) once
    assert pick[0].tolist() == [[1, 0], [0, 2], [1, 2], [-1, -1]]
    assert cand[1].tolist() == [[2, 3], [2, 1], [2, 0], [-1, -1]]                            # (2, 3) is the plain pass's pair already
    cand, _ = sh.select_candidates(scan, anchors, 1, np.array([0, 2]), np.array([0, -1]))
    assert cand[0].tolist() == [[1, 0], [-1, -1]] and cand[1].tolist() == [[2, 3], [-1, -1]]  # no valid plain pair: nothing is added
    z = sh.scan_z(scan)
    assert np.isnan(z[0, 0, 4]) and np.isnan(z[1, 0, 4]) and z[0, 1, 0] == 4.0


def fit_arrays(B, C):
    f = {k: np.zeros((B, C)) for k in ("alpha", "ll", "d1", "d2", "ll0", "d10", "d20", "ll1", "d11", "d21", "llp", "d1p", "d2p")}
    f.update({k: np.zeros((B, C), dtype=np.int32) for k in ("n_eval", "status", "n_snp", "n_read")})
    return f


def test_decision_and_writers(m, tmp_path):
    sh, capi = m["share"], m["capi"]
    ids = ["s0", "s1", "s2"]
    cand = np.array([[[0, 1], [0, 2]], [[1, 2], [-1, -1]], [[2, 0], [2, 1]], [[-1, -1], [-1, -1]]], dtype=np.int32)
    f = fit_arrays(4, 2)
    # barcode 0: slot 1 is interior, 3 above the best singlet, with the larger share on v2
    f["ll0"][0] = [-100.0, -100.0]; f["ll1"][0] = [-150.0, -140.0]; f["ll"][0] = [-100.0, -97.0]; f["alpha"][0] = [0.0, 0.7]
    f["status"][0] = [capi.DMX_SHARE_AT_0, capi.DMX_SHARE_INTERIOR]; f["d2"][0] = [-10.0, -400.0]; f["llp"][0] = [-120.0, -98.5]
    f["n_eval"][0] = [2, 7]; f["n_snp"][0] = [40, 41]; f["n_read"][0] = [50, 52]
    # barcode 1: interior but exactly 2 above: the margin is not won; the best singlet is v2 (LL(1))
    f["ll0"][1, 0] = -60.0; f["ll1"][1, 0] = -50.0; f["ll"][1, 0] = -48.0; f["alpha"][1, 0] = 0.9; f["status"][1, 0] = capi.DMX_SHARE_INTERIOR
    f["d2"][1, 0] = 0.0
    # barcode 2: no interior pair; the first maximum in slot order holds LLK.SNG
    f["ll0"][2] = [-30.0, -30.0]; f["ll1"][2] = [-90.0, -80.0]; f["ll"][2] = [-30.0, -30.0]; f["status"][2] = capi.DMX_SHARE_AT_0
    dec = sh.decide(f, cand)
    assert dec["is_dbl"].tolist() == [True, False, False, False]
    assert dec["best"].tolist() == [1, 0, 0, -1] and dec["sng"].tolist() == [0, 2, 2, -1]
    assert dec["llk_sng"][:3].tolist() == [-100.0, -50.0, -30.0] and dec["llk_dbl"][0] == -97.0 and np.isnan(dec["llk_dbl"][2])
    assert sh.oriented(0, 2, 0.7) == (2, 0, pytest.approx(0.3)) and sh.oriented(0, 2, 0.5) == (0, 2, 0.5)
    se, lo, hi = sh.wald(0.05, -400.0)
    assert se == 0.05 and lo == 0.0 and hi == pytest.approx(0.148)
    assert all(np.isnan(x) for x in sh.wald(0.3, 0.0))
    assert sh.status_text(capi.DMX_SHARE_AT_0 | capi.DMX_SHARE_FLAT) == "AT_0,FLAT" and sh.status_text(0) == "."
    scan = np.zeros((4, 1, 3, 3)); scan[..., 1] = 3.0; scan[..., 2] = -9.0
    pick = np.array([[[0, 1], [0, 2]], [[0, 2], [-1, -1]], [[-1, -1], [-1, -1]], [[-1, -1], [-1, -1]]], dtype=np.int32)
    rows = sh.call_rows(ids, cand, pick, scan, f, dec, np.array([0, 1, 2, 1]))
    assert rows[0][0] == "DBL-s2-s0-0.300" and rows[0][1:3] == ("s2", "s0") and rows[0][11] == 1.0
    assert rows[1][0] == "SNG-s2" and rows[2][0] == "SNG-s2" and rows[3][0] == "SNG-s1" and np.isnan(rows[2][11])
    barcodes = ["B", "A", "D", "C"]
    has = np.array([True, True, True, False])
    p1, p2 = str(tmp_path / "x.share.tsv"), str(tmp_path / "x.share_scan.tsv")
    sh.write_share_tsv(p1, barcodes, ["SNG-s0", "SNG-s1", "SNG-s2", ""], has, rows)
    lines = open(p1).read().split("\n")
    assert lines[0] + "\n" == sh.SHARE_HEADER and len(lines) == 5 and [x.split("\t")[0] for x in lines[1:4]] == ["A", "B", "D"]
    t = lines[2].split("\t")
    assert t[:6] == ["B", "SNG-s0", "DBL-s2-s0-0.300", "s2", "s0", "0.3000"] and t[6] == "0.0500" and t[12] == "3.00000"
    assert t[14:] == ["7", "INTERIOR", "41", "52"] and lines[1].split("\t")[6] == "NA"
    sh.write_scan_tsv(p2, barcodes, ids, has, np.array([[0], [1], [2], [0]], dtype=np.int32), pick, scan)
    lines = open(p2).read().split("\n")
    assert lines[0] + "\n" == sh.SCAN_HEADER and [x.split("\t")[:4] for x in lines[1:4]] == [["A", "s1", "s2", "1.0000"], ["B", "s0", "s1", "1.0000"],
                                                                                           ["B", "s0", "s2", "1.0000"]]


@pytest.mark.parametrize("argv", [["--anchors", "0"], ["--anchors", "5"], ["--top", "0"], ["--top", "8"], ["--tol", "0"], ["--tol", "nan"],
                                  ["--max-iter", "0"], ["--max-iter", "201"], ["--ambient", "reads"]])
def test_command_line_errors(m, argv):
    with pytest.raises(SystemExit):
        m["share"].parse_args(["--pileup", "x", "--out", "y", *argv])


def test_command_line_defaults(m):
    a = m["share"].parse_args(["--pileup", "x", "--out", "y"])
    assert (a.anchors, a.top, a.tol, a.max_iter, a.ambient, a.alpha, a.best) == (1, 4, 1e-6, 30, "reads", [0.0, 0.5], None)


def test_share_run_argument_errors(m, prob):
    sh = m["share"]
    sp = prob["sp"]
    pl = m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads, sp.rd_totl,
                                sp.rd_pass, sp.rd_uniq)
    ids = [f"s{j}" for j in range(prob["V"])]
    for kw in (dict(anchors=5), dict(top=8), dict(tol=0.0), dict(max_iter=0), dict(start=1.0), dict(ambient="soup"), dict(rho=np.ones(3))):
        with pytest.raises(ValueError):
            sh.share_run(pl, prob["g"], ids, "unused", best="unused", barcodes=[f"c{i}" for i in range(sp.n_cells)], **kw)
    with pytest.raises(ValueError):
        sh.share_run(pl, prob["g"], ids, "unused", best="unused")


def test_struct_mirrors_match_the_c_compiler(tmp_path):
    import ctypes as C
    import subprocess
    from pathlib import Path
    from demuxlet_amd import capi
    root = Path(__file__).resolve().parents[1]
    (tmp_path / "s.c").write_text('#include "dmx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                                  'sizeof(dmx_share_scan_request), offsetof(dmx_share_scan_request, anchors), offsetof(dmx_share_scan_request, ambient), '
                                  'sizeof(dmx_share_fit_request), offsetof(dmx_share_fit_request, cand), offsetof(dmx_share_fit_request, probe), '
                                  'offsetof(dmx_share_fit_request, max_iter), sizeof(dmx_share_info), offsetof(dmx_share_info, fit_evals), '
                                  'offsetof(dmx_share_info, have_fit));return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{root / 'include'}", str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = list(map(int, subprocess.check_output([str(tmp_path / "s")], text=True).split()))
    assert got == [C.sizeof(capi.ShareScanRequest), capi.ShareScanRequest.anchors.offset, capi.ShareScanRequest.ambient.offset,
                   C.sizeof(capi.ShareFitRequest), capi.ShareFitRequest.cand.offset, capi.ShareFitRequest.probe.offset,
                   capi.ShareFitRequest.max_iter.offset, C.sizeof(capi.ShareInfo), capi.ShareInfo.fit_evals.offset, capi.ShareInfo.have_fit.offset]
    assert (capi.DMX_SHARE_INTERIOR, capi.DMX_SHARE_AT_0, capi.DMX_SHARE_AT_1, capi.DMX_SHARE_NOT_CONVERGED, capi.DMX_SHARE_FLAT,
            capi.DMX_SHARE_NONFINITE) == (R.INTERIOR, R.AT_0, R.AT_1, R.NOT_CONVERGED, R.FLAT, R.NONFINITE)
