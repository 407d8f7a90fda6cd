"""GPU: k_bgzf_inflate through dmx_inflater_*  against Python's zlib on the corpora of tests/inflate_corpus.py —
the same streams tests/test_gpu_inflate_cpu.py puts through the sanitized host build of the decoder core — and the `demuxlet` binary
with DMX_GPU_INFLATE against its default path.  One launch per test where possible; every child process has a timeout."""
import gzip
import os
import re
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import inflate_corpus as ic
import sam_vcf_synth as sv

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
BIN = ROOT / "demuxlet_amd" / "demuxlet"
GUARD, FILL = 64, 0xC3


@pytest.fixture(scope="module")
def inf():
    from demuxlet_amd import build
    from demuxlet_amd.engine import Inflater
    build.build()
    h = Inflater(device=0, max_members=4096, max_in_bytes=1 << 26, max_out_bytes=1 << 26)
    yield h
    h.close()


def guards_intact(out, ooff, olen):
    """the GUARD bytes before the first slot, between slots and after the last one still hold FILL"""
    mask = np.ones(len(out), dtype=bool)
    for o, n in zip(ooff, olen):
        mask[o:o + n] = False
    return bool((out[mask] == FILL).all())


def test_valid_corpus_one_call(inf):
    valid = ic.valid_corpus()
    got, status, info, out, ooff = inf.run([z for z, _ in valid], [len(d) for _, d in valid], guard=GUARD, fill=FILL)
    print(info)
    assert info["n_members"] == len(valid) and info["n_refused"] == 0 and info["kernel_ms"] > 0
    assert not status.any(), np.flatnonzero(status)[:10]
    bad = [i for i, ((_, d), g) in enumerate(zip(valid, got)) if g != d]
    assert not bad, bad[:10]
    assert guards_intact(out, ooff, [len(d) for _, d in valid])


def test_damaged_corpus_one_call(inf):
    """2 048 damaged streams that the sanitized host build has been through: status 0 => zlib accepts at exactly out_len with these bytes;
    nothing outside a member's own range is written; and the device decides as the host build of the same core does (-O2 here)."""
    damaged = ic.damaged_corpus()
    got, status, info, out, ooff = inf.run([z for z, _ in damaged], [n for _, n in damaged], guard=GUARD, fill=FILL)
    print(info)
    assert guards_intact(out, ooff, [n for _, n in damaged])
    n_acc = 0
    for (z, n), g, s in zip(damaged, got, status):
        if s == 0:
            ok, o = ic.zlib_verdict(z, n)
            assert ok and o == g
            n_acc += 1
    assert 0 < n_acc < len(damaged) and info["n_accepted"] == n_acc


def test_device_and_host_core_decide_alike(inf, tmp_path):
    damaged = ic.damaged_corpus()
    exe = tmp_path / "inflate_core_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", str(ROOT / "demuxlet_amd" / "csrc"), str(ROOT / "tests" / "inflate_core_check.cpp"), "-o", str(exe), "-lz"],
                   check=True, timeout=120)
    ic.write_corpus(tmp_path / "c.bin", damaged)
    subprocess.run([str(exe), str(tmp_path / "c.bin"), str(tmp_path / "s.bin")], check=True, capture_output=True, timeout=120)
    host = np.frombuffer((tmp_path / "s.bin").read_bytes(), dtype=np.uint8).astype(np.int32)
    _, status, _, _, _ = inf.run([z for z, _ in damaged], [n for _, n in damaged])
    assert (status == host).all(), np.flatnonzero(status != host)[:10]


def test_longest_distance(inf):
    """Hand-made <length 258, distance 32 768> (zlib's deflate never emits it): after 32 768 bytes the copy starts at the member's byte 0 and
    walks 258 bytes over five lane strides; after 40 000 further in; after 32 767 it is one byte too far back and refused, as zlib refuses it."""
    ok, bad = ic.far_match_streams()
    assert len(ok) == 4 and len(bad) == 2 and not any(ic.zlib_verdict(z, n)[0] for z, n in bad)
    got, status, _, out, ooff = inf.run([z for z, _ in ok] + [z for z, _ in bad], [len(d) for _, d in ok] + [n for _, n in bad], guard=GUARD, fill=FILL)
    assert status[:4].tolist() == [0, 0, 0, 0] and status[4] != 0 and status[5] != 0
    assert got[:4] == [d for _, d in ok]
    assert guards_intact(out, ooff, [len(d) for _, d in ok] + [n for _, n in bad])


def chosen_members():
    """64 members: valid ones of every kind of block and size class, and damaged ones (refusals must be independent too)"""
    valid, damaged = ic.valid_corpus(), ic.damaged_corpus()
    rng = np.random.default_rng(3)
    pick = [(z, len(d)) for z, d in (valid[i] for i in rng.choice(len(valid), 48, replace=False))]
    pick += [damaged[i] for i in rng.choice(len(damaged), 14, replace=False)]
    pick += [(b"\x03\x00", 0), (valid[-1][0], len(valid[-1][1]))]
    return pick


def test_members_are_independent(inf):
    """status and bytes of 64 chosen members: alone, at n = 1, 63, 64, 65, 256 and 1 000, in reversed order, and through slot 0 and slot 1
    with both in flight — identical every time.  (The bytes of a REFUSED member are unspecified by the contract — what it did not write is
    whatever the batch buffer held — so for those the status alone is compared.)"""
    pick = chosen_members()
    assert len(pick) == 64
    filler = [(z, len(d)) for z, d in ic.valid_corpus()[::7] if len(d) <= 4096]

    def run(members):
        got, status, _, _, _ = inf.run([z for z, _ in members], [n for _, n in members])
        return [(st, g if st == 0 else None) for st, g in zip(status.tolist(), got)]

    ref = run(pick)                                                     # n = 64
    assert sum(s == 0 for s, _ in ref) >= 48 and any(s != 0 for s, _ in ref)
    for i in (0, 17, 63):                                               # alone (n = 1)
        assert run([pick[i]]) == [ref[i]]
    assert run(pick[:63]) == ref[:63]
    assert run(pick[::-1]) == ref[::-1]
    for n in (65, 256, 1000):                                           # the 64 at scattered positions among other members
        members = [filler[k % len(filler)] for k in range(n)]
        pos = np.sort(np.random.default_rng(n).choice(n, 64, replace=False))
        for p, m in zip(pos, pick):
            members[p] = m
        res = run(members)
        assert [res[p] for p in pos] == ref
    # both slots in flight: the first half through slot 0 and, reversed, the whole set through slot 1
    a, b = pick[:32], pick[::-1]
    bufs = []
    for slot, members in ((0, a), (1, b)):
        buf, off, ln = inf.pack([z for z, _ in members])
        ol = np.array([n for _, n in members], dtype=np.int32)
        ooff = np.concatenate([[0], np.cumsum(ol.astype(np.int64))[:-1]]).astype(np.int64)
        out = np.zeros(int(ol.sum()) + 1, dtype=np.uint8)
        inf.submit(slot, buf, off, ln, out, ooff, ol)
        bufs.append((out, ooff, ol))
    for slot, want in ((1, ref[::-1]), (0, ref[:32])):
        status, _ = inf.wait(slot)
        out, ooff, ol = bufs[slot]
        assert [(st, out[o:o + n].tobytes() if st == 0 else None) for st, o, n in zip(status.tolist(), ooff, ol)] == want


def test_a_member_over_the_size_limit_is_refused_not_an_error(inf):
    """in_len > 65 536 + 64 (65 536 bytes in stored blocks of 100) and out_len > 65 536: a status, the bytes untouched, the neighbours fine"""
    data = ic.make_data(0, 65536)
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    big = b"".join(c.compress(data[i:i + 100]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, 65536, 100)) + c.flush()
    assert len(big) > 65536 + 64 and zlib.decompress(big, -15) == data
    small = ic.deflate_raw(data[:1000], 6, zlib.Z_DEFAULT_STRATEGY)
    got, status, info, out, ooff = inf.run([small, big, small, small], [1000, 65536, 1000, 65537], guard=GUARD, fill=FILL)
    assert status[0] == 0 and status[2] == 0 and status[1] != 0 and status[3] != 0
    assert got[0] == data[:1000] and got[2] == data[:1000]
    assert got[1] == bytes([FILL]) * 65536 and got[3] == bytes([FILL]) * 65537
    assert guards_intact(out, ooff, [1000, 65536, 1000, 65537]) and info["n_refused"] == 2


@pytest.fixture(scope="module")
def scan_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gzscan")
    rng = np.random.default_rng(12)
    contigs = [("1", 60000), ("2", 30000)]
    recs = sv.make_vcf(rng, contigs, 400, ["a", "b", "c"], d / "v.vcf.gz", with_noise=True)
    (d / "v.vcf.gz").write_bytes(sv.bgzf_compress(gzip.open(d / "v.vcf.gz").read(), block=8000))
    sv.make_reads(rng, contigs, recs, 30000, [f"BC{i:03d}-1" for i in range(60)], d / "r.sam", d / "r.bam")
    raw = bytearray((d / "r.bam").read_bytes())
    raw[len(raw) // 2] ^= 0x10
    (d / "bad.bam").write_bytes(bytes(raw))
    return d


def demuxlet(d, out, env, sam="r.bam", pileup_only=True):
    e = {k: v for k, v in os.environ.items() if k not in ("DMX_GPU_INFLATE", "DMX_CLI_TIMING", "DMX_THREADS")}
    cmd = [str(BIN), "--sam", str(d / sam), "--vcf", str(d / "v.vcf.gz"), "--field", "GT", "--out", str(d / out)] + (["--pileup-only"] if pileup_only else [])
    return subprocess.run(cmd, capture_output=True, text=True, env={**e, **env}, timeout=120)       # a fresh child process


FIELDS = r"GPU inflate: members on device (\d+), on host (\d+), refused (\d+), device busy ([0-9.]+) s, H2D (\d+) bytes, D2H (\d+) bytes"


def test_binary_scan_is_the_same_with_the_device_stage(scan_files):
    """--pileup-only dumps with DMX_GPU_INFLATE=1 (host until the inflater is up: at 6 threads the first members arrive before it) and
    =2 (the reader waits for it, so members do go to the device) against the default path, DMX_THREADS 1 and 6."""
    d = scan_files
    base = demuxlet(d, "base", {})
    assert base.returncode == 0 and "GPU inflate" not in base.stderr
    want = (d / "base.pileup.txt").read_bytes()
    assert len(want) > 1000
    n_members = None
    for threads in ("1", "6"):
        for mode in ("1", "2"):
            name = f"g{mode}t{threads}"
            r = demuxlet(d, name, {"DMX_GPU_INFLATE": mode, "DMX_THREADS": threads, "DMX_CLI_TIMING": "1"})
            assert r.returncode == 0, r.stderr[-2000:]
            assert "GPU inflate unavailable" not in r.stderr
            assert (d / f"{name}.pileup.txt").read_bytes() == want
            m = re.search(FIELDS, r.stderr)
            assert m, r.stderr[-1500:]
            on_dev, on_host = int(m.group(1)), int(m.group(2))
            print(name, m.group(0))
            n_members = n_members or on_dev + on_host
            assert on_dev + on_host == n_members > 0                    # wherever they went, every member of both files is counted once
            if mode == "2":
                assert on_dev > 0 and int(m.group(5)) > 0 and int(m.group(6)) > 0


def test_binary_full_run_is_the_same_with_the_device_stage(scan_files):
    d = scan_files
    outs = {}
    for name, env in (("fbase", {}), ("fgpu", {"DMX_GPU_INFLATE": "2"})):
        r = demuxlet(d, name, env, pileup_only=False)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = [(d / f"{name}.{ext}").read_bytes() for ext in ("best", "single", "sing2")]
    assert all(len(b) > 100 for b in outs["fbase"]) and outs["fbase"] == outs["fgpu"]


def test_binary_reports_a_damaged_member_with_the_device_stage(scan_files):
    r = demuxlet(scan_files, "bad", {"DMX_GPU_INFLATE": "2"}, sam="bad.bam")
    assert r.returncode != 0 and "BGZF" in r.stderr
