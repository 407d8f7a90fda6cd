"""Times the joint genotype tables (k_kin_rows and k_kin_tile, dmx_engine_geno_compare) as a self-comparison at
(V, S) = (16, 100 000), (32, 50 000), (256, 100 000), (1 024, 100 000): soft float32 rows made on the device, passed as device
pointers, no weight.  Both kernels' HIP-event times (dmx_kin_info), median of --reps calls after --warmup; the tile kernel's achieved
FP64 TFLOP/s (2 * 16 * V * V * S over its time) and its fraction of the 78.6 TFLOP/s FP64 vector peak.  Beside it, at the shapes of
--matmul-shapes (the first three by default), the wall time of the same (4V x S) . (S x 4V) float64 product by numpy.matmul on the host's
threads, median of 3 after one warm-up, in the same process.  The small panels are in on purpose: one ascending chain per entry leaves
V * V * 16 chains, and at V = 16 that is 4 wavefronts of 16 fma per SNP each (about 4 issue cycles per fma) on a chip of 1 024 SIMDs.
One JSON line per shape is appended to --out.

    python tools/bench_kin.py [--reps 5] [--warmup 2] [--out profiles/kin_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
FP64_VECTOR_TFLOPS = 78.6
SHAPES = [(16, 100_000), (32, 50_000), (256, 100_000), (1024, 100_000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", type=int, nargs="+", default=None, help="V S pairs (default: the four of the docstring)")
    ap.add_argument("--matmul-shapes", type=int, default=3, help="time numpy.matmul at the first N shapes")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kin_bench.jsonl"))
    a = ap.parse_args()
    shapes = SHAPES if a.shapes is None else list(zip(a.shapes[0::2], a.shapes[1::2]))
    import torch
    from demuxlet_amd import build, capi, engine
    build.build()
    assert torch.cuda.is_available(), "bench_kin needs a GPU"
    dev = torch.device("cuda", 0)
    for k, (V, S) in enumerate(shapes):
        gen = torch.Generator(device=dev); gen.manual_seed(0x4B1 + V)
        g = torch.rand((S, V, 3), dtype=torch.float32, device=dev, generator=gen) ** 4        # soft rows, mostly on one genotype
        torch.cuda.synchronize()
        e = engine.Engine(V)
        rows_ms, tile_ms, wall_ms, info = [], [], [], None
        for _ in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            T, nv, _ = e.geno_compare(g.data_ptr(), None, None, memory=capi.DMX_MEM_DEVICE, n_snps=S, n_a=V)
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            info = e.geno_compare_info()
            rows_ms.append(info["rows_ms"]); tile_ms.append(info["tile_ms"])
        e.close()
        med = lambda xs: statistics.median(xs[a.warmup:])
        tf = info["flop"] / med(tile_ms) / 1e9
        row = dict(V=V, S=S, reps=a.reps, warmup=a.warmup, tile_a=info["tile_a"], tile_b=info["tile_b"], chunk_snps=info["chunk_snps"],
                   workgroups=-(-V // info["tile_a"]) * -(-V // info["tile_b"]), flop=info["flop"], bytes=info["bytes"],
                   rows_ms=round(med(rows_ms), 3), tile_ms=round(med(tile_ms), 3), tile_ms_min=round(min(tile_ms[a.warmup:]), 3),
                   tile_ms_max=round(max(tile_ms[a.warmup:]), 3), call_wall_ms=round(med(wall_ms), 1),
                   fp64_tflops=round(tf, 3), fp64_vector_peak_share=round(tf / FP64_VECTOR_TFLOPS, 4),
                   rows_gb_per_s=round((12 + 32) * 2 * S * V / med(rows_ms) / 1e6, 1), n_valid_min=int(nv.min()))
        if k < a.matmul_shapes:
            gd = g.double()
            p = (gd / gd.sum(dim=2, keepdim=True)).cpu().numpy()
            del gd
            img = np.concatenate([p, np.ones((S, V, 1))], axis=2).reshape(S, 4 * V)            # [S][4V], the B image; A = its transpose
            at = np.ascontiguousarray(img.T)
            ts = []
            for _ in range(4):
                t0 = time.perf_counter()
                ref = at @ img
                ts.append((time.perf_counter() - t0) * 1e3)
            row.update(numpy_matmul_ms=round(statistics.median(ts[1:]), 1), numpy_threads=os.environ.get("OMP_NUM_THREADS", "unset"),
                       numpy_over_tile=round(statistics.median(ts[1:]) / med(tile_ms), 1),
                       max_rel_diff_to_numpy=float(np.max(np.abs(ref.reshape(V, 4, V, 4).transpose(0, 2, 1, 3) - T) / np.maximum(np.abs(T), 1e-300))))
            del p, img, at, ref
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        print(json.dumps(row), flush=True)
        del g, T
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
