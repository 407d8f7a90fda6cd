"""CPU: dmx_log2 of a MIRRORED pair (x, x') — the alpha-0.5 sums of the doublet entries [j][k] and [k][j], one number up to a few ulp — returns the bits of
two independent dmx_log2_core calls.  The mirrored form (csrc/dmx_log.hpp) takes the exponent, the table entry, kd and w from the primary x when the high
words agree from bit 11 up, and evaluates the mirror whole otherwise; the STRICT unordered-pair doublet kernels call it in phase 2.  Here: the host side of
the same header (g++, -ffp-contract=off, libm's fma), on
  (a) test_dmx_log.sample_points_k2's points paired with themselves and with their +-1 .. +-4 ulp neighbours,
  (b) pairs that straddle each of the 256 bin edges (the exponent edge among them) by one ulp, in four exponents and both orders,
  (c) pairs that straddle the high word's bit-11 step in the middle of a bin, likewise.
The guard must report the whole evaluation for every pair of (b) and (c), and for fewer than 1 % of (a)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import log_mirror_points as pts

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    so = tmp_path_factory.mktemp("logmirror") / "liblogmirror.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", f"-I{ROOT / 'demuxlet_amd' / 'csrc'}",
                           str(ROOT / "tests" / "log_mirror_emul.cpp"), "-o", str(so), "-lm"])
    L = C.CDLL(str(so))
    L.dmx_log2_whole_n.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    L.dmx_log2_mirror_n.argtypes = [C.c_void_p] * 5 + [C.c_long]

    def whole(x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        L.dmx_log2_whole_n(x.ctypes.data, y.ctypes.data, len(x))
        return y

    def run(x, xm):
        """asserts the property; returns the guard's verdict per pair"""
        x, xm = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(xm, dtype=np.float64)
        y, ym, fb = np.empty_like(x), np.empty_like(x), np.empty(len(x), dtype=np.int32)
        L.dmx_log2_mirror_n(x.ctypes.data, xm.ctypes.data, y.ctypes.data, ym.ctypes.data, fb.ctypes.data, len(x))
        for got, arg, what in ((y, x, "primary"), (ym, xm, "mirror")):
            want = whole(arg)
            bad = got.view(np.uint64) != want.view(np.uint64)
            assert not bad.any(), f"{what}: {bad.sum()} of {len(x)} differ, first at x = {x[bad][0].hex()}, x' = {xm[bad][0].hex()}"
        return fb != 0
    return run


def test_points_and_their_ulp_neighbours(mirror):
    x, xm = pts.ordinary_pairs(np.random.default_rng(811), 20000)
    fell_back = mirror(x, xm)
    assert fell_back.mean() < 0.01, f"{fell_back.sum()} of {len(x)} pairs left the shared evaluation"
    same = x.view(np.uint64) == xm.view(np.uint64)
    assert not fell_back[same].any()                           # a bit-equal mirror (the diagonal units of k_doublet_a2u2) never does


def test_pairs_across_every_bin_edge(mirror):
    x, xm = pts.bin_edge_pairs()
    assert len(x) == 2 * 256 * len(pts.EXPONENTS) and np.all(pts.bin_of(x) != pts.bin_of(xm))      # (the exponent edge: bin 0 against the exponent below's bin 255)
    assert np.all(np.abs(x.view(np.int64) - xm.view(np.int64)) == 1)
    assert mirror(x, xm).all()


def test_pairs_across_a_bit11_step_inside_a_bin(mirror):
    x, xm = pts.mid_bin_step_pairs()
    assert np.all(pts.bin_of(x) == pts.bin_of(xm)) and np.all(np.abs(x.view(np.int64) - xm.view(np.int64)) == 1)
    assert mirror(x, xm).all()                                 # sufficient, not necessary: a false alarm, and still the same bits
