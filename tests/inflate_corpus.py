"""Raw-DEFLATE corpora for the device inflater's tests (tests/test_gpu_inflate_cpu.py, tests/test_gpu_inflate.py), made with Python's
zlib at wbits = -15 and seeded, so that the CPU test (the sanitized host build of dmx_inflate_core.hpp) and the GPU test (k_bgzf_inflate)
see exactly the same streams.

valid_corpus()     tests/inflate_check.cpp's shape — six data kinds x 13 sizes x five levels x four strategies = 1 560 streams — and more
                   sizes, Z_FIXED, level 0 (stored), several blocks (Z_FULL_FLUSH between writes), a kind with geometric symbol
                   frequencies (15-bit codes, second-level tables), far matches (distance 32 000 from zlib; hand-made distance 32 768 with length 258,
                   far_match_streams), overlapped copies at distances 1-7.
damaged_corpus()   single-bit flips, truncations and wrong out_len (n - 1, n + 1, 0) of valid streams, capped.
zlib_verdict()     whether zlib accepts a stream at exactly out_len bytes, and the bytes.
write_corpus()     the file format tests/inflate_core_check.cpp reads: u32 in_len, u32 out_len, in_len bytes, per stream."""
import functools
import struct
import zlib

import numpy as np

SIZES = (0, 1, 2, 7, 64, 287, 288, 289, 300, 1000, 4096, 65280, 65536)
MORE_SIZES = (0, 1, 2, 63, 64, 65, 257, 258, 259, 288, 289, 4095, 4096, 4097, 65535, 65536)
LEVELS = (0, 1, 4, 6, 9)
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)
MAX_IN, MAX_OUT = 65536 + 64, 65536


@functools.lru_cache(maxsize=None)
def make_data(kind: int, n: int) -> bytes:
    rng = np.random.default_rng(1000 * kind + n % 997)
    if kind == 0:                                           # incompressible
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == 1:                                           # four symbols
        return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
    if kind == 2:                                           # short periods: distances 1..7
        out = bytearray()
        while len(out) < n:
            pat = rng.integers(0, 256, int(rng.integers(1, 8)), dtype=np.uint8).tobytes()
            out += (pat * 48)[:int(rng.integers(8, 300))]
        return bytes(out[:n])
    if kind == 3:                                           # one long run (distance 1, length 258)
        return bytes(n)
    if kind == 4:                                           # BAM-like: short repeats + noisy bytes
        out = bytearray()
        while len(out) < n:
            if len(out) > 300 and rng.integers(0, 4):
                ln, dist = int(rng.integers(3, 15)), int(rng.integers(1, 301))
                for _ in range(ln):
                    out.append(out[-dist])
            else:
                out += (33 + rng.integers(0, 42, int(rng.integers(1, 6)), dtype=np.uint8)).astype(np.uint8).tobytes()
        return bytes(out[:n])
    if kind == 5:                                           # structured, long matches far back
        i = np.arange(n, dtype=np.uint64)
        return (((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(13)).astype(np.uint8).tobytes()
    if kind == 6:                                           # geometric symbol frequencies: codes of up to 15 bits
        return np.minimum(rng.geometric(0.5, n) - 1, 40).astype(np.uint8).tobytes()
    if kind == 7:                                           # a 32 000-byte period: zlib's deflate finds matches of length 258 at distance 32 000
        base = rng.integers(0, 256, 32000, dtype=np.uint8).tobytes()      # (its own limit is 32 768 - 262; distance 32 768 itself is hand-made below)
        return (base * (n // 32000 + 1))[:n]
    raise ValueError(kind)


def deflate_raw(data: bytes, level: int, strategy: int, pieces: int = 1) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    out = b""
    for q in range(pieces):
        lo, hi = len(data) * q // pieces, len(data) * (q + 1) // pieces
        out += c.compress(data[lo:hi])
        if q + 1 < pieces:
            out += c.flush(zlib.Z_FULL_FLUSH)
    return out + c.flush()


def far_match_block(extra: int = 8191) -> bytes:
    """A final fixed-code block, starting at a byte boundary: <length 258, distance 24 577 + extra>, end of block.  extra = 8 191 is the
    longest distance DEFLATE can say: 32 768 (symbol 29, all 13 extra bits set)."""
    bits = []
    put = lambda v, n: bits.extend((v >> i) & 1 for i in range(n))                  # header fields and extra bits: LSB first
    code = lambda c, n: bits.extend((c >> i) & 1 for i in range(n - 1, -1, -1))     # Huffman codes: MSB first
    put(1, 1); put(1, 2)                                    # BFINAL, BTYPE = fixed
    code(0b11000101, 8)                                     # symbol 285: length 258, no extra bits
    code(29, 5); put(extra, 13)                             # distance symbol 29
    code(0, 7)                                              # end of block
    bits += [0] * (-len(bits) % 8)
    return bytes(sum(b << i for i, b in enumerate(bits[k:k + 8])) for k in range(0, len(bits), 8))


def far_match_streams():
    """Hand-made streams around the longest distance (zlib's deflate never emits one above 32 768 - 262, so none of its streams gets there):
    -> (accepted, refused), lists of (deflate bytes, data or out_len).
    accepted: 32 768 and 40 000 bytes — in a stored block, and deflated by zlib up to a Z_SYNC_FLUSH — then <258, 32 768>: with 32 768 bytes
    the copy starts at the member's byte 0.  refused: the same after 32 767 bytes (one byte too far back; zlib rejects it too)."""
    ok, bad = [], []
    for n in (32768, 40000, 32767):
        p = make_data(0, n)
        stored = struct.pack("<BHH", 0, n, n ^ 0xFFFF) + p
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        packed = c.compress(p) + c.flush(zlib.Z_SYNC_FLUSH)
        for z in (stored + far_match_block(), packed + far_match_block()):
            if n >= 32768:
                ok.append((z, p + p[n - 32768:n - 32768 + 258]))
            else:
                bad.append((z, n + 258))
    return ok, bad


@functools.lru_cache(maxsize=1)
def valid_corpus():
    """-> tuple of (deflate bytes, data bytes)"""
    v = []
    for kind in range(6):
        for n in SIZES:
            d = make_data(kind, n)
            for level in LEVELS:
                for strategy in STRATEGIES:
                    v.append((deflate_raw(d, level, strategy), d))
    assert len(v) == 6 * 13 * 5 * 4
    for kind in (1, 2, 4, 6):
        for n in MORE_SIZES:
            d = make_data(kind, n)
            v += [(deflate_raw(d, 6, zlib.Z_DEFAULT_STRATEGY), d), (deflate_raw(d, 6, zlib.Z_FIXED), d), (deflate_raw(d, 0, zlib.Z_DEFAULT_STRATEGY), d),
                  (deflate_raw(d, 9, zlib.Z_DEFAULT_STRATEGY, 5), d)]
    for n in (40000, 65536):
        for level in (1, 6, 9):
            z7 = deflate_raw(make_data(7, n), level, zlib.Z_DEFAULT_STRATEGY)
            assert len(z7) < 36000                          # the far matches were found: not stored
            v.append((z7, make_data(7, n)))
            v.append((deflate_raw(make_data(6, n), level, zlib.Z_HUFFMAN_ONLY, 3), make_data(6, n)))
    for dist in range(1, 8):                                # overlapped copies at every distance 1..7
        d = (bytes(range(97, 97 + dist)) * 3000)[:3000]
        v.append((deflate_raw(d, 9, zlib.Z_DEFAULT_STRATEGY), d))
    v += far_match_streams()[0]                             # distance 32 768, length 258
    assert all(len(z) <= MAX_IN and len(d) <= MAX_OUT for z, d in v)
    return tuple(v)


def zlib_verdict(z: bytes, out_len: int):
    """(accepted, bytes): zlib inflates z to a stream end after exactly out_len bytes (input left over does not matter)"""
    d = zlib.decompressobj(-15)
    try:
        o = d.decompress(z, out_len + 1)
    except zlib.error:
        return False, b""
    return (d.eof and len(o) == out_len), o


@functools.lru_cache(maxsize=4)
def damaged_corpus(cap: int = 2048, seed: int = 7):
    """-> tuple of (deflate bytes, out_len): `cap` seeded damages of valid streams — 70 % one flipped bit, 10 % a truncation, 20 % a
    wrong out_len (n - 1, n + 1, 0).  Streams of more than 8 KiB of data are taken less often, to keep the device batch small."""
    rng = np.random.default_rng(seed)
    valid = [s for s in valid_corpus() if len(s[0]) > 0]
    small = [s for s in valid if len(s[1]) <= 8192]
    out = []
    while len(out) < cap:
        pool = small if rng.random() < 0.9 else valid
        z, d = pool[int(rng.integers(0, len(pool)))]
        r = rng.random()
        if r < 0.7:
            b = bytearray(z)
            b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
            out.append((bytes(b), len(d)))
        elif r < 0.8:
            if len(z) > 1:
                out.append((z[:int(rng.integers(1, len(z)))], len(d)))
        elif r < 0.87:
            if len(d) > 0:
                out.append((z, len(d) - 1))
        elif r < 0.94:
            if len(d) < MAX_OUT:
                out.append((z, len(d) + 1))
        elif len(d) > 0:
            out.append((z, 0))
    return tuple(out)


def write_corpus(path, streams) -> None:
    """streams: iterable of (deflate bytes, out_len)"""
    with open(path, "wb") as f:
        for z, n in streams:
            f.write(struct.pack("<II", len(z), n))
            f.write(z)
