"""Times the ambient-aware doublet profile (dmx_engine_ambient_doublet, k_ambient_dbl) at cfg3 (dense, 10k x 50k x 32, GP) and cfg6
(sparse, 20k x 100k x 16, ~2 000 SNPs per barcode) for (C, A) = (1, 1), (2, 1), (2, 5), (8, 1) on the default 51-point grid, and in the
same process, alternating with it, the unchanged k_ambient on the same pileup and grid as the yardstick.  HIP-event times, median of
--reps calls after --warmup.  Candidate c of a barcode is (truth + c, truth + c + 1) mod V.  Prints one JSON line per configuration and
(C, A); `est_ratio` is the instruction-count estimate 2.4 + (C - 1) / 3 per alpha of DESIGN.md section 18.

    python tools/bench_ambient_dbl.py [--configs 3 6] [--reps 10] [--warmup 2] [--grid-points 51]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = [(1, 1), (2, 1), (2, 5), (8, 1)]
ALPHAS = {1: [0.5], 5: [0.1, 0.2, 0.3, 0.4, 0.5]}


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
        t0 = assign.cpu().numpy().astype(np.int32)
        amb = np.clip(raw.alleles, 0, 1).sum(axis=2).mean(axis=1) / 2.0
        torch.cuda.synchronize()
        e = engine.Engine(V, cfg["alphas"], 0.5)
        e.set_genotypes(g)
        e.set_pileup_struct(dp.as_struct(), keep=dp)
        for Cn, An in SHAPES:
            cand = np.stack([np.stack([(t0 + c) % V, (t0 + c + 1) % V], axis=1) for c in range(Cn)], axis=1).astype(np.int32)
            d_cand = torch.from_numpy(cand).to(dev)
            dbl, sng = [], []
            for i in range(a.warmup + a.reps):
                e.ambient_doublet_profile(int(d_cand.data_ptr()), ALPHAS[An], amb, grid, n_cand=Cn)
                dbl.append(e.ambient_doublet_info()["kernel_ms"])
                e.ambient_profile(int(assign.data_ptr()), amb, grid)
                sng.append(e.ambient_info()["kernel_ms"])
            dbl, sng = dbl[a.warmup:], sng[a.warmup:]
            md, ms = statistics.median(dbl), statistics.median(sng)
            est = An * (2.4 + (Cn - 1) / 3.0)
            print(json.dumps(dict(config=cfg_id, B=B, S=S, V=V, pairs=dp.n_pairs, reads=dp.n_reads, grid_points=len(grid), n_cand=Cn, n_alpha=An,
                                  reps=len(dbl), ambient_dbl_ms=round(md, 3), ambient_dbl_ms_min=round(min(dbl), 3),
                                  ambient_dbl_ms_max=round(max(dbl), 3), ambient_ms=round(ms, 3), ambient_ms_min=round(min(sng), 3),
                                  ambient_ms_max=round(max(sng), 3), ratio=round(md / ms, 3), est_ratio=round(est, 3),
                                  ratio_over_est=round(md / ms / est, 3))), flush=True)
        e.close()
        del dp, dosage, assign
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
