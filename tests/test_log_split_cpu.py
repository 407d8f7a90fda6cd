"""CPU: dmx_log2 in two parts — dmx_log2_request (integer extraction and the table read), then dmx_log2_finish (the arithmetic) —
returns dmx_log2_core's bits.  The STRICT unordered-pair doublet kernel issues the four requests of a unit together and runs the four
second parts behind one LDS wait; this is the proof that the split itself moves no bit.  Points: test_dmx_log.py's own vectors (every
bin edge of both reductions and its neighbours, the whole exponent range, random mantissas, the neighbourhood of 1)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_dmx_log import sample_points_k2

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    so = tmp_path_factory.mktemp("logsplit") / "liblogsplit.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", f"-I{ROOT / 'demuxlet_amd' / 'csrc'}",
                           str(ROOT / "tests" / "log_split_emul.cpp"), "-o", str(so), "-lm"])
    L = C.CDLL(str(so))
    for f in (L.dmx_log2_whole_n, L.dmx_log2_split_n):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_long]

    def run(x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        whole, parts = np.empty_like(x), np.empty_like(x)
        L.dmx_log2_whole_n(x.ctypes.data, whole.ctypes.data, len(x))
        L.dmx_log2_split_n(x.ctypes.data, parts.ctypes.data, len(x))
        return whole, parts
    return run


def test_request_then_finish_is_dmx_log2_bit_for_bit(split):
    rng = np.random.default_rng(613)
    x = sample_points_k2(rng, 100000)
    whole, parts = split(x)
    assert np.array_equal(whole.view(np.uint64), parts.view(np.uint64)), f"{np.sum(whole.view(np.uint64) != parts.view(np.uint64))} of {len(x)} differ"


def test_every_exponent_and_special_arguments(split):
    """One mantissa sweep in every binary exponent of the normal range, and the arguments that leave the fast path (both forms hand them to libm)."""
    rng = np.random.default_rng(614)
    m = np.concatenate([[0.5, np.nextafter(1.0, 0)], rng.uniform(0.5, 1.0, 14)])
    x = np.ldexp(m[None, :], np.arange(-1021, 1025)[:, None]).ravel()
    whole, parts = split(x)
    assert np.array_equal(whole.view(np.uint64), parts.view(np.uint64))
    with np.errstate(all="ignore"):
        whole, parts = split(np.array([0.0, -1.0, np.inf, np.nan, 5e-324, 2.2250738585072014e-308]))
    assert np.array_equal(whole.view(np.uint64), parts.view(np.uint64))
    assert parts[0] == -np.inf and np.isnan(parts[1]) and parts[2] == np.inf and np.isnan(parts[3])
