"""CPU: the list of used barcodes that dmx_engine_fit, dmx_engine_site_fit and dmx_engine_redraw share
(demuxlet_amd/csrc/dmx_hyp_plan.hpp, through tests/hyp_plan_shim.cpp): its order is the site audit's sum order (include/dmx.h), and
its check is the three calls' bad-hypothesis error.  g++ alone: no HIP, no GPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
V = 7


@pytest.fixture(scope="module")
def lister(tmp_path_factory):
    so = tmp_path_factory.mktemp("hyp_plan") / "libhyp_plan_shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", f"-I{ROOT / 'demuxlet_amd' / 'csrc'}",
                           str(ROOT / "tests" / "hyp_plan_shim.cpp"), "-o", str(so)])
    L = C.CDLL(str(so))
    L.hyp_plan_list.restype = C.c_int32
    L.hyp_plan_list.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(hyp, n_samples=V):
        """(first bad barcode or -1, the list, the number of singlets in it)"""
        hyp = np.ascontiguousarray(hyp, dtype=np.int32).reshape(-1, 2)
        B = hyp.shape[0]
        idx = np.full(max(B, 1), -7, dtype=np.int32)
        n_used, n_sng = C.c_int32(-1), C.c_int32(-1)
        bad = L.hyp_plan_list(hyp.ctypes.data if B else None, B, n_samples, idx.ctypes.data, C.byref(n_used), C.byref(n_sng))
        return bad, idx[:n_used.value].copy(), n_sng.value

    return run


def random_mix(rng, B):
    """hyp [B][2]: about a third each of unused (-1, anything), singlet (v, -1) and doublet (v1, v2 != v1) hypotheses."""
    hyp = np.full((B, 2), -1, dtype=np.int32)
    kind = rng.integers(0, 3, size=B)
    for b in range(B):
        if kind[b] == 0:
            hyp[b, 1] = rng.integers(-3, V + 3)                    # ignored where the first entry is -1
        else:
            hyp[b, 0] = rng.integers(0, V)
            if kind[b] == 2:
                hyp[b, 1] = (hyp[b, 0] + rng.integers(1, V)) % V
    return hyp, kind


def restated(hyp):
    b = np.arange(hyp.shape[0], dtype=np.int32)
    sng = b[(hyp[:, 0] >= 0) & (hyp[:, 1] < 0)]
    dbl = b[(hyp[:, 0] >= 0) & (hyp[:, 1] >= 0)]
    return np.concatenate([sng, dbl]), len(sng)


@pytest.mark.parametrize("B", [0, 1, 130])
def test_list_is_singlets_then_doublets_ascending(lister, B):
    rng = np.random.default_rng(100 + B)
    for _ in range(1 if B == 0 else 6):
        hyp, kind = random_mix(rng, B)
        bad, idx, n_sng = lister(hyp)
        want, want_sng = restated(hyp)
        assert bad == -1
        assert n_sng == want_sng == int((kind == 1).sum())
        assert np.array_equal(idx, want)
        assert (np.diff(idx[:n_sng]) > 0).all() and (np.diff(idx[n_sng:]) > 0).all()
    if B == 130:
        assert 0 < n_sng < len(idx) < B                           # all three kinds were there


def test_one_barcode_of_each_kind(lister):
    assert [list(lister([[-1, -1]])[1]), lister([[-1, -1]])[2]] == [[], 0]
    assert [list(lister([[-1, 3]])[1]), lister([[-1, 3]])[2]] == [[], 0]
    assert [list(lister([[2, -1]])[1]), lister([[2, -1]])[2]] == [[0], 1]
    assert [list(lister([[2, 5]])[1]), lister([[2, 5]])[2]] == [[0], 0]


@pytest.mark.parametrize("pair", [(V, -1), (-2, -1), (0, V), (1, 1), (0, -2)])
def test_bad_hypothesis_is_refused_at_the_first_offender(lister, pair):
    rng = np.random.default_rng(7)
    hyp, _ = random_mix(rng, 130)
    assert lister(hyp)[0] == -1
    for at in (0, 57, 129):
        h = hyp.copy()
        h[at] = pair
        assert lister(h)[0] == at
    h = hyp.copy()
    h[90] = (V, V)                                                 # a later offender of another kind does not move the report
    h[33] = pair
    assert lister(h)[0] == 33
