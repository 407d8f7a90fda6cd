"""Measures the device inflater on the BGZF members of tools/make_cli_bench.py's BAM and the `demuxlet`
binary's scan with and without DMX_GPU_INFLATE; appends JSON lines to profiles/gpu_inflate_bench.jsonl.

    python tools/bench_gpu_inflate.py [--reads 2000000] [--dir DIR] [--batch 256 1024] [--skip-e2e]

kernel      HIP events around k_bgzf_inflate (dmx_inflater_info.kernel_ms), 2 warm-ups, median of 5 and the spread: output GB/s, members/s
pipeline    submit -> wait wall-clock of consecutive batches through the two slots (H2D + kernel + D2H overlapped), whole file
host        the binary's own DMX_CLI_TIMING inflate CPU-seconds (dmx_inflate.hpp on the host's threads)
end to end  the binary's scan timing, default path and DMX_GPU_INFLATE=1 alternating, five runs each, dumps compared md5 for md5;
            the baseline is the default path."""
import argparse
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def bgzf_members(path):
    """-> list of (deflate bytes, isize) of every member"""
    raw = Path(path).read_bytes()
    out, at = [], 0
    while at < len(raw):
        xlen = struct.unpack_from("<H", raw, at + 10)[0]
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1          # make_cli_bench.py / bgzip: BC is the first extra field
        out.append((raw[at + 12 + xlen:at + bsize - 8], struct.unpack_from("<I", raw, at + bsize - 4)[0]))
        at += bsize
    return out


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def bench_kernel(inf, members, batch):
    from demuxlet_amd.engine import Inflater
    m = members[:batch]
    buf, off, ln = Inflater.pack([z for z, _ in m])
    ol = np.array([n for _, n in m], dtype=np.int32)
    ooff = np.concatenate([[0], np.cumsum(ol.astype(np.int64))[:-1]]).astype(np.int64)
    out = np.zeros(int(ol.sum()) + 1, dtype=np.uint8)
    L = inf._L
    for a in (buf, out):
        L.dmx_inflater_pin(a.ctypes.data, a.nbytes)
    ks, ws, hs, ds = [], [], [], []
    for rep in range(7):
        t0 = time.perf_counter()
        inf.submit(0, buf, off, ln, out, ooff, ol)
        status, info = inf.wait(0)
        w = time.perf_counter() - t0
        assert not status.any()
        if rep >= 2:
            ks.append(info["kernel_ms"]); ws.append(1e3 * w); hs.append(info["h2d_ms"]); ds.append(info["d2h_ms"])
    for a in (buf, out):
        L.dmx_inflater_unpin(a.ctypes.data)
    nbytes = int(ol.sum())
    k = stats(ks)
    return {"what": "kernel", "batch_members": len(m), "out_bytes": nbytes, "in_bytes": int(ln.sum()), "kernel_ms": k, "h2d_ms": stats(hs), "d2h_ms": stats(ds),
            "submit_to_wait_ms": stats(ws), "kernel_out_GBps": nbytes / k["median"] / 1e6, "kernel_members_per_s": len(m) / k["median"] * 1e3,
            "submit_to_wait_out_GBps": nbytes / stats(ws)["median"] / 1e6}


def bench_pipeline(inf, members, batch):
    """the whole file through the two slots, as the scanner drives them"""
    from demuxlet_amd.engine import Inflater
    batches = []
    for lo in range(0, len(members), batch):
        m = members[lo:lo + batch]
        buf, off, ln = Inflater.pack([z for z, _ in m])
        ol = np.array([n for _, n in m], dtype=np.int32)
        ooff = np.concatenate([[0], np.cumsum(ol.astype(np.int64))[:-1]]).astype(np.int64)
        batches.append((buf, off, ln, ol, ooff))
    outs = [np.zeros(batch * 65536 + 1, dtype=np.uint8) for _ in range(2)]
    L = inf._L
    for a in outs:
        L.dmx_inflater_pin(a.ctypes.data, a.nbytes)
    walls = []
    for rep in range(7):
        t0 = time.perf_counter()
        for i, (buf, off, ln, ol, ooff) in enumerate(batches):
            if i >= 2:
                status, _ = inf.wait(i & 1)
                assert not status.any()
            inf.submit(i & 1, buf, off, ln, outs[i & 1], ooff, ol)
        for i in range(max(0, len(batches) - 2), len(batches)):
            status, _ = inf.wait(i & 1)
            assert not status.any()
        if rep >= 2:
            walls.append(time.perf_counter() - t0)
    for a in outs:
        L.dmx_inflater_unpin(a.ctypes.data)
    nbytes = sum(n for _, n in members)
    w = stats(walls)
    return {"what": "pipeline", "batch_members": batch, "n_members": len(members), "out_bytes": nbytes, "wall_s": w, "out_GBps": nbytes / w["median"] / 1e9,
            "members_per_s": len(members) / w["median"], "note": "input staging is pageable here (numpy); the scanner's is page-locked"}


def scan_once(d, name, env):
    e = {k: v for k, v in os.environ.items() if k not in ("DMX_GPU_INFLATE",)}
    t0 = time.perf_counter()
    r = subprocess.run([str(ROOT / "demuxlet_amd" / "demuxlet"), "--sam", f"{d}/bench.bam", "--vcf", f"{d}/bench.vcf", "--field", "GT", "--out", f"{d}/{name}",
                        "--pileup-only"], capture_output=True, text=True, env={**e, "DMX_CLI_TIMING": "1", **env}, timeout=900)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"scan timing \((\d+) threads, \w+\): total ([0-9.]+) s = ([0-9.e+]+) reads/s", r.stderr)
    c = re.search(r"process CPU so far: ([0-9.]+) s user \+ ([0-9.]+) s system; inside the parallel sections: inflate ([0-9.]+) s", r.stderr)
    g = re.search(r"GPU inflate: members on device (\d+), on host (\d+), refused (\d+), device busy ([0-9.]+) s, H2D (\d+) bytes, D2H (\d+) bytes", r.stderr)
    row = {"threads": int(m.group(1)), "scan_s": float(m.group(2)), "reads_per_s": float(m.group(3)), "cpu_user_s": float(c.group(1)), "cpu_sys_s": float(c.group(2)),
           "inflate_cpu_s": float(c.group(3)), "process_wall_s": wall, "md5": hashlib.md5(Path(f"{d}/{name}.pileup.txt").read_bytes()).hexdigest()}
    if g:
        row.update(members_on_device=int(g.group(1)), members_on_host=int(g.group(2)), members_refused=int(g.group(3)), device_busy_s=float(g.group(4)),
                   h2d_bytes=int(g.group(5)), d2h_bytes=int(g.group(6)))
    return row


def bench_e2e(d, reads):
    rows = {"default": [], "gpu_inflate": []}
    scan_once(d, "warm", {})                                           # the file cache
    for rep in range(5):                                               # alternating, five each
        rows["default"].append(scan_once(d, "o_default", {}))
        rows["gpu_inflate"].append(scan_once(d, "o_gpu", {"DMX_GPU_INFLATE": "1"}))
    md5 = {r["md5"] for rs in rows.values() for r in rs}
    assert len(md5) == 1, md5
    out = {"what": "end_to_end", "reads": reads, "dumps_agree": True, "baseline": "default path (DMX_GPU_INFLATE unset)"}
    for k, rs in rows.items():
        out[k] = {f: stats([r[f] for r in rs]) for f in ("scan_s", "reads_per_s", "cpu_user_s", "cpu_sys_s", "inflate_cpu_s", "process_wall_s")}
        if "members_on_device" in rs[0]:
            out[k]["timing_fields"] = [{f: r[f] for f in ("members_on_device", "members_on_host", "members_refused", "device_busy_s", "h2d_bytes", "d2h_bytes")} for r in rs]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--batch", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gpu_inflate_bench.jsonl"))
    a = ap.parse_args()
    from demuxlet_amd import build
    from demuxlet_amd.engine import Inflater
    build.build()
    d = a.dir or os.path.join(os.environ.get("TMPDIR", "/tmp"), f"dmx_gz_bench_{a.reads}")
    os.makedirs(d, exist_ok=True)
    rows = []
    if not os.path.exists(f"{d}/bench.bam"):
        t0 = time.perf_counter()
        subprocess.run([sys.executable, str(ROOT / "tools" / "make_cli_bench.py"), d, str(a.reads), "60000", "16", "3000"], check=True)
        rows.append({"what": "generate", "reads": a.reads, "seconds": time.perf_counter() - t0})
    members = bgzf_members(f"{d}/bench.bam")
    rows.append({"what": "data", "reads": a.reads, "n_members": len(members), "deflate_bytes": sum(len(z) for z, _ in members), "inflated_bytes": sum(n for _, n in members)})
    inf = Inflater(0, max(a.batch), max(a.batch) * (65536 + 128), max(a.batch) * 65536)
    for b in a.batch:
        rows.append(bench_kernel(inf, members, b))
        rows.append(bench_pipeline(inf, members, b))
    inf.close()
    if not a.skip_e2e:
        rows.append(bench_e2e(d, a.reads))
    with open(a.out, "a") as f:
        for r in rows:
            r["reads"] = a.reads
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
