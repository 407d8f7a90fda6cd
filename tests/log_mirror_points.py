"""Argument pairs (x, x') for the mirrored dmx_log2 (csrc/dmx_log.hpp), shared by test_log_mirror_cpu.py and test_gpu_log_mirror.py.

dmx_log2 reduces x = 2^k z with z in [OFF2, 2 OFF2), OFF2's high word 0x3FE5F800, and takes the bin from bits 12..19 of hi(x) - 0x3FE5F800: a bin edge is a
double whose high word ends in 0x800 and whose low word is zero, the exponent edge is bin 0's.  The mirrored form shares the primary's table entry when
hi(x) ^ hi(x') < 0x800; the high word's bit 11 also steps in the middle of a bin (high word ending in 0x000), where the guard fails although the bin is one."""
import numpy as np

from test_dmx_log import sample_points_k2

OFF2 = 0x3FE5F80000000000
EXPONENTS = (-20, -3, 0, 1)          # binary exponents k of the edge sets: likelihood terms (1e-6, 0.1), the reduced range itself, above 1


def neighbours(x, d):
    return (x.view(np.int64) + d).view(np.float64)


def ordinary_pairs(rng, n):
    """(a) sample_points_k2's points (positive normal ones) with themselves and with their +-1 .. +-4 ulp neighbours."""
    x = sample_points_k2(rng, n)
    x = x[(x > 1e-305) & (x < 1e305)]
    return np.concatenate([x] * 9), np.concatenate([neighbours(x, d) for d in (0, 1, -1, 2, -2, 3, -3, 4, -4)])


def _straddles(first_hi_low12):
    bits = np.array([OFF2 - 0x80000000000 + (first_hi_low12 << 32) + (i << 44) + (k << 52) for k in EXPONENTS for i in range(256)], dtype=np.int64)
    up, down = bits.view(np.float64), (bits - 1).view(np.float64)
    return np.concatenate([up, down]), np.concatenate([down, up])


def bin_edge_pairs():
    """(b) every one of the 256 bin edges (bin 0's is the exponent edge) in four exponents: the edge and the double below it, in both orders."""
    return _straddles(0x800)


def mid_bin_step_pairs():
    """(c) the high word's step ...FFF -> ...000 in the middle of every bin, same exponents: one bin, but bit 11 (and more) of the high words differ."""
    return _straddles(0x1000)


def bin_of(x):
    """(exponent, bin) of dmx_log2's reduction."""
    tmp = ((x.view(np.uint64) >> np.uint64(32)).astype(np.int64) - 0x3FE5F800) & 0xFFFFFFFF
    return tmp >> 12
