"""Times the ambient contamination profile (dmx_engine_ambient) at cfg3 (dense, 10k x 50k x 32, GP) and cfg6 (sparse, 20k x 100k x 16,
~2 000 SNPs per barcode): bench.py's panels and device pileups, every barcode assigned from truth, the default 51-point grid, HIP-event
time of k_ambient (median of --reps calls after --warmup).  Prints one JSON line per configuration.

    python tools/bench_ambient.py [--configs 3 6] [--reps 10] [--warmup 2] [--grid-points 51]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[3, 6])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grid-points", type=int, default=51)
    a = ap.parse_args()
    import torch
    import bench
    from demuxlet_amd import build, engine, synth, synth_torch
    build.build()
    dev = torch.device("cuda", 0)
    grid = np.arange(a.grid_points) * 0.01
    for cfg_id in a.configs:
        cfg = bench.CONFIGS[cfg_id]
        B, S, V = cfg["B"], cfg["S"], cfg["V"]
        rng = np.random.default_rng(0xD3A00000 + cfg_id)
        raw, g = bench.genotype_matrix(engine, synth, rng, S, V, cfg["field"])
        dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
        dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xD3A0 + 1000 * cfg_id, device=dev)
        assign = dp.truth[:, 0].contiguous()
        amb = np.clip(raw.alleles, 0, 1).sum(axis=2).mean(axis=1) / 2.0
        torch.cuda.synchronize()
        e = engine.Engine(V, cfg["alphas"], 0.5)
        e.set_genotypes(g)
        e.set_pileup_struct(dp.as_struct(), keep=dp)
        infos = []
        for i in range(a.warmup + a.reps):
            e.ambient_profile(int(assign.data_ptr()), amb, grid)
            infos.append(e.ambient_info())
        e.close()
        timed = [x["kernel_ms"] for x in infos[a.warmup:]]
        print(json.dumps(dict(config=cfg_id, name=cfg["name"], B=B, S=S, V=V, pairs=dp.n_pairs, reads=dp.n_reads, grid_points=len(grid),
                              reps=len(timed), ambient_ms=round(statistics.median(timed), 3), ambient_ms_min=round(min(timed), 3),
                              ambient_ms_max=round(max(timed), 3), profile_bytes=infos[0]["profile_bytes"])), flush=True)
        del dp, dosage, assign
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
