"""Times the genotype-free clustering (dmx_engine_cluster_*) at cfg6 size (sparse, 20k barcodes x 100k SNPs, ~2 000 covered SNPs per
barcode, K = 16) and cfg3 size (dense, 10k x 50k, K = 32), R = 4 restarts: bench.py's device pileups of K donors, the stage once, then
--iters EM iterations as cluster.cluster_run runs them (set_genotypes from the device, K1, E-step, M-step).  Per iteration: K1's
HIP-event time (the E-step's likelihoods), the E-step's and the M-step's; plus the stage time and the cache's bytes.  One JSON line
per configuration, also appended to --out.

    python tools/bench_cluster.py [--configs 6 3] [--iters 6] [--out profiles/cluster_bench.jsonl]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SHAPES = {6: 16, 3: 32}      # config -> K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[6, 3])
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--restarts", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from demuxlet_amd import build, cluster, engine, synth, synth_torch
    build.build()
    dev = torch.device("cuda", 0)
    for cfg_id in a.configs:
        cfg = bench.CONFIGS[cfg_id]
        B, S, K, R = cfg["B"], cfg["S"], SHAPES[cfg_id], a.restarts
        C = R * K
        rng = np.random.default_rng(0xC0000000 + cfg_id)
        raw = synth.make_raw_genotypes(rng, S, K)
        dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
        dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xC0C0 + cfg_id, device=dev)
        torch.cuda.synchronize()
        e = engine.Engine(C, cfg["alphas"], 0.5)
        e.set_genotypes(np.full((S, C, 3), 1.0 / 3.0, dtype=np.float32))
        e.set_pileup_struct(dp.as_struct(), keep=dp)
        e.cluster_stage()
        st = e.cluster_info()
        q = cluster.hwe_prior(np.zeros(S), np.zeros(S))
        t0 = time.perf_counter()
        e.cluster_mstep(cluster.one_hot_weights(cluster.initial_labels(0, R, B, K), K), q, fetch=False)
        log_pi = np.full((R, K), -np.log(K))
        its = []
        for it in range(a.iters):
            t1 = time.perf_counter()
            e.set_genotypes_device(e.cluster_device_ptr(), S)
            if dp.pair_snp is None:
                e.set_pileup_struct(dp.as_struct(), keep=dp)
            e.run_singlet()
            ll, cs = e.cluster_estep(R, K, log_pi)
            k1 = e.kernel_times().singlet_ms
            log_pi = cluster.update_log_pi(cs, R, K)
            e.cluster_mstep(None, q, fetch=False)
            inf = e.cluster_info()
            its.append(dict(k1_ms=k1, estep_ms=inf["estep_ms"], mstep_ms=inf["mstep_ms"], wall_ms=1e3 * (time.perf_counter() - t1)))
        total = time.perf_counter() - t0
        e.close()
        rec = dict(config=cfg_id, name=cfg["name"], B=B, S=S, K=K, R=R, columns=C, layout="dense" if dp.pair_snp is None else "sparse",
                   pairs=dp.n_pairs, reads=dp.n_reads, stage_ms=round(st["stage_ms"], 3), cache_bytes=st["cache_bytes"],
                   scratch_bytes=st["scratch_bytes"], iters=a.iters,
                   k1_ms_median=round(statistics.median(x["k1_ms"] for x in its[1:] or its), 3),
                   estep_ms_median=round(statistics.median(x["estep_ms"] for x in its[1:] or its), 3),
                   mstep_ms_median=round(statistics.median(x["mstep_ms"] for x in its[1:] or its), 3),
                   iteration_wall_ms_median=round(statistics.median(x["wall_ms"] for x in its[1:] or its), 3),
                   per_iteration=[{k: round(v, 3) for k, v in x.items()} for x in its], em_wall_s=round(total, 3))
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del dp, dosage
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
