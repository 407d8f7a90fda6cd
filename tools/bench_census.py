"""Times the donor-share census (dmx_engine_census_step / dmx_engine_census) at cfg6 (sparse, 20k x 100k x 16, ~2 000 SNPs per barcode) and
cfg3 (dense, 10k x 50k x 32, GP): bench.py's panels and device pileups, every barcode in one group and in 16 groups (cell id mod 16),
uniform shares.  Per configuration and group count: the HIP-event time of one pass (k_census_step + k_census_fold; median of --reps
calls after --warmup), the engine's own K1 time on the same pileup (mean_kernel_times after --reps run_singlet calls) and their ratio;
then the steps and wall time of a whole driver run (SQUAREM, default tolerance).  Prints one JSON line per measurement and appends it
to profiles/census_bench.jsonl.

    python tools/bench_census.py [--configs 6 3] [--groups 1 16] [--reps 10] [--warmup 2] [--no-driver] [--out profiles/census_bench.jsonl]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[6, 3])
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-driver", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "census_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import bench
    from demuxlet_amd import build, engine, synth, synth_torch
    build.build()
    dev = torch.device("cuda", 0)

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    for cfg_id in a.configs:
        cfg = bench.CONFIGS[cfg_id]
        B, S, V = cfg["B"], cfg["S"], cfg["V"]
        rng = np.random.default_rng(0xCE500000 + cfg_id)
        raw, g = bench.genotype_matrix(engine, synth, rng, S, V, cfg["field"])
        dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
        dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xCE50 + 1000 * cfg_id, device=dev)
        torch.cuda.synchronize()
        e = engine.Engine(V, cfg["alphas"], 0.5)
        e.set_genotypes(g)
        e.set_pileup_struct(dp.as_struct(), keep=dp)
        e.reset_kernel_times()
        for _ in range(a.reps):
            e.run_singlet()
        e.sync()
        k1 = e.mean_kernel_times()
        k1_ms = float(k1.singlet_ms)
        for G in a.groups:
            group = torch.arange(B, dtype=torch.int32, device=dev) % G
            w = np.full((G, V), 1.0 / V)
            infos = []
            for _ in range(a.warmup + a.reps):
                e.census_step(int(group.data_ptr()), w, n_groups=G)
                infos.append(e.census_info())
            timed = [x["kernel_ms"] for x in infos[a.warmup:]]
            med = statistics.median(timed)
            emit(what="step", config=cfg_id, name=cfg["name"], B=B, S=S, V=V, pairs=dp.n_pairs, reads=dp.n_reads, groups=G, reps=len(timed),
                 step_ms=round(med, 3), step_ms_min=round(min(timed), 3), step_ms_max=round(max(timed), 3), k1_ms=round(k1_ms, 3),
                 k1_launches=int(k1.n_singlet), step_over_k1=round(med / k1_ms, 3) if k1_ms > 0 else None,
                 ns_per_pair=round(med * 1e6 / max(dp.n_pairs, 1), 4), dosage_ms=round(infos[-1]["dosage_ms"], 3),
                 n_chunks=infos[-1]["n_chunks"], partial_bytes=infos[-1]["partial_bytes"], dosage_bytes=infos[-1]["dosage_bytes"])
            if not a.no_driver:
                t0 = time.perf_counter()
                r = e.census(int(group.data_ptr()), n_groups=G)
                wall = time.perf_counter() - t0
                emit(what="driver", config=cfg_id, B=B, S=S, V=V, groups=G, passes=e.census_info()["n_steps"],
                     steps_min=int(r["n_steps"].min()), steps_max=int(r["n_steps"].max()), converged=int(r["converged"].sum()),
                     gap_max=float(r["gap"].max()), wall_s=round(wall, 3))
            del group
        e.close()
        del dp, dosage
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
