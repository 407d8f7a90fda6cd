"""CPU: the device inflater's decoder core (demuxlet_amd/csrc/dmx_inflate_core.hpp, the code k_bgzf_inflate instantiates) as a host
program under AddressSanitizer + UBSan and at -O2 (tests/inflate_core_check.cpp: stand-alone, exact-size heap buffers, against zlib);
the same program over the seeded Python corpus that tests/test_gpu_inflate.py gives the device; dmx_inflater_create and the
`demuxlet` binary's DMX_GPU_INFLATE=1 on a host without a GPU."""
import gzip
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import inflate_corpus as ic
import sam_vcf_synth as sv

ROOT = Path(__file__).resolve().parents[1]
BIN = ROOT / "demuxlet_amd" / "demuxlet"
NOTICE = "GPU inflate unavailable ("
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build_check(tmp_path, flags):
    exe = tmp_path / "inflate_core_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", str(ROOT / "demuxlet_amd" / "csrc"), str(ROOT / "tests" / "inflate_core_check.cpp"), "-o", str(exe),
                    "-lz"], check=True)
    return exe


def no_gpu():
    import torch
    return not torch.cuda.is_available()


@pytest.mark.parametrize("flags", [SAN, ["-O2"]], ids=["sanitized", "O2"])
def test_core_against_zlib(tmp_path, flags):
    """Valid corpus: every stream accepted with zlib's bytes.  Damaged corpus: status 0 => zlib accepts the stream at exactly out_len
    with the same bytes; each of the classes 'zlib rejects' and 'zlib accepts with other bytes' is at least a quarter of it (the program
    checks that itself and counts it as a failure)."""
    exe = build_check(tmp_path, flags)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"valid streams ok (\d+) of (\d+), failures (\d+)", r.stdout)
    assert m and m.group(1) == m.group(2) and m.group(3) == "0"
    assert int(m.group(1)) >= 6 * 13 * 5 * 4 + 3 + 200          # inflate_check.cpp's shape, the hand-made three, and the added streams
    m = re.search(r"damaged (\d+): zlib rejects (\d+), zlib accepts with the original bytes (\d+), zlib accepts with other bytes (\d+); core accepted (\d+); failures 0", r.stdout)
    assert m, r.stdout
    n, rej, same, other, acc = map(int, m.groups())
    assert n >= 4 * 1560 and 4 * rej >= n and 4 * other >= n
    assert acc <= same + other
    assert r.stdout.rstrip().endswith("failures 0")


def test_python_corpus_through_the_sanitized_core(tmp_path):
    """The corpus of tests/test_gpu_inflate.py — the valid streams and the 2 048 damaged ones — through the sanitized host build first:
    no report, every valid stream accepted, and of the damaged ones status 0 only with zlib's bytes (the program asks the C zlib; the
    classes are counted here with Python's)."""
    exe = build_check(tmp_path, SAN)
    valid, damaged = ic.valid_corpus(), ic.damaged_corpus()
    far_ok, far_bad = ic.far_match_streams()                  # hand-made <length 258, distance 32 768>: at byte 0, further in, one byte too far
    assert len(valid) >= 1560 + 200 and len(damaged) == 2048 and all(s in valid for s in far_ok) and len(far_bad) == 2
    damaged = tuple(far_bad) + damaged
    ic.write_corpus(tmp_path / "corpus.bin", [(z, len(d)) for z, d in valid] + list(damaged))
    r = subprocess.run([str(exe), str(tmp_path / "corpus.bin"), str(tmp_path / "status.bin")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-600:], r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"file streams {len(valid) + len(damaged)}," in r.stdout and "failures 0" in r.stdout
    st = np.frombuffer((tmp_path / "status.bin").read_bytes(), dtype=np.uint8)
    assert len(st) == len(valid) + len(damaged)
    assert not st[:len(valid)].any()
    assert st[len(valid)] != 0 and st[len(valid) + 1] != 0 and not any(ic.zlib_verdict(z, n)[0] for z, n in far_bad)
    rejects = other = 0
    orig = {}
    for z, d in valid:
        orig.setdefault(len(d), set()).add(d)
    for (z, n), s in zip(damaged, st[len(valid):]):
        ok, o = ic.zlib_verdict(z, n)
        assert ok or s != 0, (len(z), n, int(s))       # status 0 => zlib accepts (the converse is not promised: a refusal goes to zlib)
        rejects += not ok
        other += ok and o not in orig.get(n, ())
    assert 4 * rejects >= len(damaged) and 4 * other >= len(damaged), (rejects, other)


def test_inflater_create_without_a_gpu():
    if not no_gpu():
        pytest.skip("a GPU is present")
    import ctypes as C
    from demuxlet_amd import build, capi
    from demuxlet_amd.engine import Inflater
    build.build()
    lib = capi.load()
    h = C.c_void_p()
    assert lib.dmx_inflater_create(0, 256, 1 << 24, 1 << 24, C.byref(h)) == -5 and not h.value
    assert b"no HIP device" in lib.dmx_last_error()
    with pytest.raises(capi.DmxError) as ei:
        Inflater()
    assert ei.value.code == -5
    assert lib.dmx_inflater_create(0, 0, 1 << 24, 1 << 24, C.byref(h)) == -1          # arguments are checked before the device is looked for
    buf = np.zeros(4096, np.uint8)
    assert lib.dmx_inflater_pin(buf.ctypes.data, 4096) < 0 and lib.dmx_inflater_free(None) == 0


@pytest.fixture(scope="module")
def scan_files(tmp_path_factory):
    from demuxlet_amd import build
    build.build()
    d = tmp_path_factory.mktemp("gzscan")
    rng = np.random.default_rng(11)
    contigs = [("1", 60000), ("2", 30000)]
    recs = sv.make_vcf(rng, contigs, 400, ["a", "b", "c"], d / "v.vcf.gz", with_noise=True)
    (d / "v.vcf.gz").write_bytes(sv.bgzf_compress(gzip.open(d / "v.vcf.gz").read(), block=8000))     # bgzipped: BGZF members, not one gzip member
    sv.make_reads(rng, contigs, recs, 30000, [f"BC{i:03d}-1" for i in range(60)], d / "r.sam", d / "r.bam")
    return d


def scan(d, out, sam, env):
    e = {k: v for k, v in os.environ.items() if k not in ("DMX_GPU_INFLATE", "DMX_CLI_TIMING")}
    return subprocess.run([str(BIN), "--sam", str(d / sam), "--vcf", str(d / "v.vcf.gz"), "--field", "GT", "--out", str(d / out), "--pileup-only"],
                          capture_output=True, text=True, env={**e, **env}, timeout=120)


def test_binary_without_a_device_inflates_on_the_host(scan_files):
    """DMX_GPU_INFLATE=1 where no device is usable: one notice, the host path's bytes, exit status 0 — for the BAM and for the bgzipped
    VCF (both are BGZF here) and for SAM text with the bgzipped VCF alone.  Without the variable nothing mentions the stage."""
    if not no_gpu():
        pytest.skip("a GPU is present")
    d = scan_files
    base = scan(d, "base", "r.bam", {})
    assert base.returncode == 0 and "GPU inflate" not in base.stderr
    want = (d / "base.pileup.txt").read_bytes()
    assert len(want) > 1000
    for name, sam, env in (("g1", "r.bam", {"DMX_GPU_INFLATE": "1"}), ("g1t1", "r.bam", {"DMX_GPU_INFLATE": "1", "DMX_THREADS": "1"}),
                           ("g2", "r.bam", {"DMX_GPU_INFLATE": "2", "DMX_CLI_TIMING": "1"}), ("g1sam", "r.sam", {"DMX_GPU_INFLATE": "1"})):
        r = scan(d, name, sam, env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr.count(NOTICE) == 1 and "): BGZF members are inflated on the host" in r.stderr
        assert (d / f"{name}.pileup.txt").read_bytes() == want
        if "DMX_CLI_TIMING" in env:
            m = re.search(r"GPU inflate: members on device (\d+), on host (\d+), refused (\d+), device busy ([0-9.]+) s, H2D (\d+) bytes, D2H (\d+) bytes", r.stderr)
            assert m and int(m.group(1)) == 0 and int(m.group(2)) > 0 and int(m.group(5)) == 0
    off = scan(d, "off", "r.bam", {"DMX_GPU_INFLATE": "0", "DMX_CLI_TIMING": "1"})
    assert off.returncode == 0 and "GPU inflate" not in off.stderr and (d / "off.pileup.txt").read_bytes() == want


def test_binary_without_a_device_still_reports_a_damaged_member(scan_files):
    if not no_gpu():
        pytest.skip("a GPU is present")
    d = scan_files
    raw = bytearray((d / "r.bam").read_bytes())
    raw[len(raw) // 2] ^= 0x10
    (d / "bad.bam").write_bytes(bytes(raw))
    r = scan(d, "bad", "bad.bam", {"DMX_GPU_INFLATE": "1"})
    assert r.returncode != 0 and "BGZF" in r.stderr
