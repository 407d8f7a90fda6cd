"""Times k_block_col (dmx_engine_block_llk) at G = 1, 40 and 400 blocks of equal SNP count with E = 2 extra entries per barcode and, in
the same process on the same pileup, k_anchor_col — the existing kernel that evaluates column 0 of the grid without blocks
(dmx_engine_doublet_anchored with T = 1 and the caller's anchors, so that its col_ms holds k_anchor_col and a 4 B-byte upload, no
k_anchor_select).  HIP-event times; the median of 5 runs after 2 warm-ups, minimum and maximum stated.  One process per shape.  Shapes:
cfg6 and cfg3.  The figure: the time per evaluated entry (k_block_col: V + A + E per barcode; k_anchor_col: V A + A) relative to
k_anchor_col's, and how it moves with G; the zeroing of the results is timed apart (zero_ms).  Prints one JSON line per shape and
appends it to profiles/blocks_bench.jsonl.

    python tools/bench_blocks.py [--shapes cfg6 cfg3] [--no-append]"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = {"cfg6": 6, "cfg3": 3}
BLOCKS = (1, 40, 400)
N_EXTRA = 2
REPS, WARMUPS = 5, 2


def stats(ms):
    ms = np.asarray(ms[WARMUPS:])
    return dict(ms=round(float(np.median(ms)), 3), ms_min=round(float(ms.min()), 3), ms_max=round(float(ms.max()), 3))


def run_shape(name: str, append: bool) -> None:
    import torch
    import bench
    from demuxlet_amd import build, engine, synth, synth_torch
    build.build()
    dev = torch.device("cuda", 0)
    cfg_id = SHAPES[name]
    cfg = bench.CONFIGS[cfg_id]
    B, S, V, A = cfg["B"], cfg["S"], cfg["V"], len(cfg["alphas"])
    rng = np.random.default_rng(0xB10C0000 + cfg_id)
    raw, g = bench.genotype_matrix(engine, synth, rng, S, V, cfg["field"])
    dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
    dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xB10C + 1000 * cfg_id, device=dev)
    del dosage, raw
    torch.cuda.synchronize()
    e = engine.Engine(V, cfg["alphas"], 0.5, mode=engine.capi.DMX_MODE_STRICT)
    e.set_genotypes(g)
    e.set_pileup_struct(dp.as_struct(), keep=dp)
    row = dict(shape=name, B=B, S=S, V=V, A=A, E=N_EXTRA, pairs=int(dp.n_pairs), reads=int(dp.n_reads), reps=REPS, warmups=WARMUPS)
    anchors = np.zeros((B, 1), dtype=np.int32)
    ms = []
    for _ in range(REPS + WARMUPS):
        e.doublet_anchored(anchors=anchors)
        ms.append(e.anchored_info()["col_ms"])
    ent_a = V * A + A
    row["anchor_col"] = dict(stats(ms), entries_per_barcode=ent_a)
    ns_a = row["anchor_col"]["ms"] * 1e6 / (B * ent_a)
    row["anchor_col"]["ns_per_entry"] = round(ns_a, 4)
    b = np.arange(B)
    extra = np.stack([np.stack([b % V, (b + 1) % V, np.full(B, A - 1)], axis=1), np.stack([(b + 1) % V, b % V, np.full(B, A - 1)], axis=1)],
                     axis=1).astype(np.int32)
    ent_b = V + A + N_EXTRA
    for G in BLOCKS:
        block = ((np.arange(S, dtype=np.int64) * G) // S).astype(np.int32)
        ms, zs = [], []
        for _ in range(REPS + WARMUPS):
            e.block_llk(block, G, extra)
            inf = e.block_llk_info()
            ms.append(inf["kernel_ms"]); zs.append(inf["zero_ms"])
        r = dict(stats(ms), zero_ms=stats(zs)["ms"], entries_per_barcode=ent_b, result_bytes=int(inf["result_bytes"]))
        r["ns_per_entry"] = round(r["ms"] * 1e6 / (B * ent_b), 4)
        r["per_entry_ratio_to_anchor_col"] = round(r["ns_per_entry"] / ns_a, 4)
        r["time_ratio_to_anchor_col"] = round(r["ms"] / row["anchor_col"]["ms"], 4)
        row[f"G{G}"] = r
    e.close()
    line = json.dumps(row)
    print(line, flush=True)
    if append:
        with open(ROOT / "profiles" / "blocks_bench.jsonl", "a") as f:
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
