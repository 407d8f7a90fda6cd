"""Times the genotype refinement (dmx_engine_refine_genotypes) at cfg3 (dense, 10k x 50k x 32, GP) and cfg6 (sparse, 20k x 100k x 16,
~2 000 SNPs per barcode): bench.py's panels and device pileups, every barcode assigned from truth, HIP-event times of the refine kernels
(median of --reps calls after --warmup), and the partial buffer's size.  Prints one JSON line per configuration.

    python tools/bench_refine.py [--configs 3 6] [--reps 10] [--warmup 2]"""
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
    a = ap.parse_args()
    import torch
    import bench
    from demuxlet_amd import build, engine, synth, synth_torch
    build.build()
    dev = torch.device("cuda", 0)
    for cfg_id in a.configs:
        cfg = bench.CONFIGS[cfg_id]
        B, S, V = cfg["B"], cfg["S"], cfg["V"]
        rng = np.random.default_rng(0xD3A00000 + cfg_id)
        raw, g = bench.genotype_matrix(engine, synth, rng, S, V, cfg["field"])
        dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
        dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xD3A0 + 1000 * cfg_id, device=dev)
        assign = dp.truth[:, 0].contiguous()
        torch.cuda.synchronize()
        e = engine.Engine(V, cfg["alphas"], 0.5)
        e.set_genotypes(g)
        e.set_pileup_struct(dp.as_struct(), keep=dp)
        infos = []
        for i in range(a.warmup + a.reps):
            e.refine_genotypes(int(assign.data_ptr()), g)
            infos.append(e.refine_info())
        e.close()
        first, timed = infos[0], infos[a.warmup:]
        part = statistics.median(x["partial_ms"] for x in timed)
        fin = statistics.median(x["finish_ms"] for x in timed)
        tot = statistics.median(x["partial_ms"] + x["finish_ms"] for x in timed)
        print(json.dumps(dict(config=cfg_id, name=cfg["name"], B=B, S=S, V=V, pairs=dp.n_pairs, reads=dp.n_reads, reps=len(timed),
                              refine_ms=round(tot, 3), partial_fold_ms=round(part, 3), finish_ms=round(fin, 3),
                              partial_fold_ms_min=round(min(x["partial_ms"] for x in timed), 3), blocks_ms_first_call=round(first["blocks_ms"], 3),
                              partial_bytes=first["partial_bytes"], n_chunks=first["n_chunks"], n_waves=first["n_waves"],
                              chunk_cells=first["chunk_cells"], slab_snps=first["slab_snps"])), flush=True)
        del dp, dosage, assign
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
