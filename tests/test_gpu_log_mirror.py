"""GPU (-m gpu): dmx_log2 of a mirrored pair on the device (dmx_debug_device_log2_mirror: one pair per lane through the request, the finish, the wave-uniform
guard test and the out-of-line whole evaluation that the STRICT unordered-pair doublet kernels call) returns dmx_debug_device_log2's bits for each argument
alone.  Point sets: test_log_mirror_cpu.py's (log_mirror_points.py), under 1e5 pairs in all; one array alternates ordinary pairs with pairs that straddle a bin
edge or a mid-bin step of the high word, so that every wavefront holds lanes of both kinds — the branch is taken and the per-lane select has both outcomes."""
import numpy as np
import pytest

import log_mirror_points as pts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from demuxlet_amd import build, capi
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    L = capi.load()

    def alone(x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        capi.check(L.dmx_debug_device_log2(x.ctypes.data, y.ctypes.data, len(x), 0))
        return y

    def check(x, xm):
        x, xm = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(xm, dtype=np.float64)
        assert len(x) <= 100000
        y, ym = np.empty_like(x), np.empty_like(x)
        capi.check(L.dmx_debug_device_log2_mirror(x.ctypes.data, xm.ctypes.data, y.ctypes.data, ym.ctypes.data, len(x), 0))
        for got, arg, what in ((y, x, "primary"), (ym, xm, "mirror")):
            want = alone(arg)
            bad = got.view(np.uint64) != want.view(np.uint64)
            assert not bad.any(), f"{what}: {bad.sum()} of {len(x)} differ, first at x = {x[bad][0].hex()}, x' = {xm[bad][0].hex()}"
    return check


def test_points_and_their_ulp_neighbours(dev):
    x, xm = pts.ordinary_pairs(np.random.default_rng(812), 2000)      # 9 pairings of ~8 700 points
    dev(x, xm)


def test_pairs_across_every_bin_edge(dev):
    dev(*pts.bin_edge_pairs())


def test_pairs_across_a_bit11_step_inside_a_bin(dev):
    dev(*pts.mid_bin_step_pairs())


def test_straddling_and_ordinary_pairs_in_one_wavefront(dev):
    sx, sxm = (np.concatenate(a) for a in zip(pts.bin_edge_pairs(), pts.mid_bin_step_pairs()))
    ox, oxm = pts.ordinary_pairs(np.random.default_rng(813), 200)
    guard = ((ox.view(np.uint64) >> np.uint64(32)) ^ (oxm.view(np.uint64) >> np.uint64(32))) < 0x800
    ox, oxm = ox[guard][:len(sx)], oxm[guard][:len(sx)]                 # pairs that stay on the shared evaluation
    assert len(ox) == len(sx)
    x, xm = np.empty(2 * len(sx)), np.empty(2 * len(sx))
    x[0::2], xm[0::2], x[1::2], xm[1::2] = ox, oxm, sx, sxm            # every 64 consecutive elements: 32 of each kind
    dev(x, xm)
    x[0::4], xm[0::4] = sx[0::2], sxm[0::2]                            # ... and 48 straddling pairs to 16 ordinary ones
    dev(x, xm)
