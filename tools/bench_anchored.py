"""Times the anchored doublet search (dmx_engine_doublet_anchored: k_anchor_col + k_anchor_select, k_anchor_pair, k_anchor_reduce) at
T = 1, 2 and 4 anchors and, in the same process on the same pileup, the full STRICT doublet step of Engine.run() (K2 + K3 from
dmx_engine_last_kernel_times) where its grid fits the free device memory and one step stays under a minute.  HIP-event times; the median
of 10 runs after 2 warm-ups, for the full step as well.  One process per shape.  Shapes: cfg3, cfg6, cfg4's 12 500-barcode shard, and
cfg6-shaped pileups over 256 and 1 024 samples.  Prints one JSON line per shape and appends it to profiles/anchored_bench.jsonl.

    python tools/bench_anchored.py [--shapes cfg3 cfg6 cfg4shard cfg6v256 cfg6v1024] [--no-append]"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = {
    # name: (bench.CONFIGS id, overrides)
    "cfg3": (3, {}),
    "cfg6": (6, {}),
    "cfg4shard": (4, dict(B=12_500)),
    "cfg6v256": (6, dict(V=256)),
    "cfg6v1024": (6, dict(V=1024)),
}
ANCHORS = (1, 2, 4)
FULL_STEP_LIMIT_S = 60.0


def run_shape(name: str, append: bool) -> None:
    import torch
    import bench
    from demuxlet_amd import build, engine, synth, synth_torch
    build.build()
    dev = torch.device("cuda", 0)
    cfg_id, over = SHAPES[name]
    cfg = dict(bench.CONFIGS[cfg_id], **over)
    B, S, V, A = cfg["B"], cfg["S"], cfg["V"], len(cfg["alphas"])
    rng = np.random.default_rng(0xA2C40000 + cfg_id + V)
    raw, g = bench.genotype_matrix(engine, synth, rng, S, V, cfg["field"])
    dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
    dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xA2C4 + 1000 * cfg_id + V, device=dev)
    del dosage, raw
    torch.cuda.synchronize()
    e = engine.Engine(V, cfg["alphas"], 0.5, mode=engine.capi.DMX_MODE_STRICT)
    e.set_genotypes(g)
    e.set_pileup_struct(dp.as_struct(), keep=dp)
    row = dict(shape=name, B=B, S=S, V=V, A=A, pairs=int(dp.n_pairs), reads=int(dp.n_reads), reps=10, warmups=2)
    for T in ANCHORS:
        ms = []
        for i in range(12):
            e.doublet_anchored(T)
            inf = e.anchored_info()
            ms.append((inf["col_ms"], inf["pair_ms"], inf["reduce_ms"]))
        ms = np.array(ms[2:])
        med = np.median(ms, axis=0)
        row[f"T{T}"] = dict(col_ms=round(float(med[0]), 3), pair_ms=round(float(med[1]), 3), reduce_ms=round(float(med[2]), 3),
                            total_ms=round(float(np.median(ms.sum(axis=1))), 3), total_ms_min=round(float(ms.sum(axis=1).min()), 3),
                            total_ms_max=round(float(ms.sum(axis=1).max()), 3), result_bytes=int(inf["result_bytes"]),
                            entries_per_barcode=round(inf["n_entries"] / B, 1))
    grid_bytes = B * V * V * A * 8
    row["grid_bytes"] = grid_bytes
    row["full_entries_per_barcode"] = V * V * A + A
    free_b = torch.cuda.mem_get_info(0)[0]
    full = "not run"
    if grid_bytes + grid_bytes // 8 < free_b:
        ts = []
        for i in range(12):
            e.run(); e.sync()
            kt = e.kernel_times()
            ts.append(float(kt.doublet_ms) + float(kt.reduce_ms))
            if ts[-1] > FULL_STEP_LIMIT_S * 1e3:
                break
        if ts[-1] <= FULL_STEP_LIMIT_S * 1e3:
            full = round(statistics.median(ts[2:]), 3)
    row["full_strict_ms"] = full
    for T in ANCHORS:
        row[f"T{T}"]["ratio_to_full"] = round(row[f"T{T}"]["total_ms"] / full, 4) if full != "not run" else "not run"
        row[f"T{T}"]["result_over_grid_bytes"] = round(row[f"T{T}"]["result_bytes"] / grid_bytes, 5)
    e.close()
    line = json.dumps(row)
    print(line, flush=True)
    if append:
        with open(ROOT / "profiles" / "anchored_bench.jsonl", "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--no-append", action="store_true")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        run_shape(a.child, not a.no_append)
        return 0
    for name in a.shapes:                              # one process per shape: nothing of one shape's allocations or clocks carries over
        rc = subprocess.run([sys.executable, __file__, "--child", name] + (["--no-append"] if a.no_append else [])).returncode
        if rc != 0:
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
