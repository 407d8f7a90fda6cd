"""Times the census uncertainty pass (dmx_engine_census_fisher: k_census_fisher + k_census_fisher_fold) on bench.py's panels and device
pileups: cfg6 (sparse, 20k x 100k, V = 16), cfg3 (dense, 10k x 50k, V = 32, GP) and a cfg6-shaped pileup with V = 128, every barcode in
one group, uniform shares.  Per shape: the HIP-event time of the two kernels (median of --reps calls after --warmup), the time of a
k_census_step + k_census_fold pass on the same pileup measured the same way, and their ratio.  Prints one JSON line per shape and
appends it to profiles/census_fisher_bench.jsonl.

    python tools/bench_census_fisher.py [--shapes cfg6 cfg3 cfg6v128] [--reps 10] [--warmup 2] [--out profiles/census_fisher_bench.jsonl]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = {"cfg6": (6, None), "cfg3": (3, None), "cfg6v128": (6, 128)}     # bench.py's configuration, V override


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "census_fisher_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import bench
    from demuxlet_amd import build, capi, engine, synth, synth_torch
    import ctypes as C
    build.build()
    dev = torch.device("cuda", 0)
    for shape in a.shapes:
        cfg_id, v_over = SHAPES[shape]
        cfg = bench.CONFIGS[cfg_id]
        B, S, V = cfg["B"], cfg["S"], (v_over or cfg["V"])
        rng = np.random.default_rng(0xF15000 + cfg_id + (v_over or 0))
        raw, g = bench.genotype_matrix(engine, synth, rng, S, V, cfg["field"])
        dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
        dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xF150 + 1000 * cfg_id, device=dev)
        torch.cuda.synchronize()
        e = engine.Engine(V, cfg["alphas"], 0.5)
        e.set_genotypes(g)
        e.set_pileup_struct(dp.as_struct(), keep=dp)
        group = torch.zeros(B, dtype=torch.int32, device=dev)
        w = np.full((1, V), 1.0 / V)
        H = np.zeros((1, V, V))
        rq = capi.CensusFisherRequest(B, capi.DMX_MEM_DEVICE, int(group.data_ptr()), 1, V, w.ctypes.data, H.ctypes.data)   # (H only: no B x V copy)
        fis, step = [], []
        for _ in range(a.warmup + a.reps):
            capi.check(e._L.dmx_engine_census_fisher(e._h, C.byref(rq)))
            fis.append(e.census_fisher_info())
            e.census_step(int(group.data_ptr()), w, n_groups=1)
            step.append(e.census_info()["kernel_ms"])
        t_f = [x["kernel_ms"] for x in fis[a.warmup:]]
        t_s = step[a.warmup:]
        med_f, med_s = statistics.median(t_f), statistics.median(t_s)
        E = V * (V + 1) // 2
        line = json.dumps(dict(what="fisher", shape=shape, config=cfg_id, name=cfg["name"], B=B, S=S, V=V, entries=E, pairs=dp.n_pairs,
                               reads=dp.n_reads, reps=len(t_f), fisher_ms=round(med_f, 3), fisher_ms_min=round(min(t_f), 3),
                               fisher_ms_max=round(max(t_f), 3), step_ms=round(med_s, 3), fisher_over_step=round(med_f / med_s, 2) if med_s > 0 else None,
                               ps_per_pair_entry=round(med_f * 1e9 / max(dp.n_pairs * E, 1), 3), n_chunks=fis[-1]["n_chunks"],
                               n_blocks=fis[-1]["n_blocks"], partial_bytes=fis[-1]["partial_bytes"],
                               trace_H_over_N=round(float(np.trace(H[0])) / max(dp.n_reads, 1), 4)))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        e.close()
        del dp, dosage, group
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
