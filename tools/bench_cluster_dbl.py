"""Times the doublet-aware clustering's two kernels (dmx_engine_cluster_doublet: k_cluster_dbl; dmx_engine_cluster_estep_doublet:
k_cluster_estep_dbl + the ordered sums) at cfg6 size (sparse, 20k barcodes x 100k SNPs, ~2 000 covered SNPs per barcode, K = 16) and
cfg3 size (dense, 10k x 50k, K = 32), R = 4 restarts: bench.py's device pileups of K donors, the stage, one M-step from each restart's
random labels and K1 on its result, then --warmup + --reps calls of both; HIP-event times, median of the timed calls.  One JSON line
per configuration, also appended to --out.

    python tools/bench_cluster_dbl.py [--configs 6 3] [--reps 10] [--warmup 2] [--out profiles/cluster_dbl_bench.jsonl]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SHAPES = {6: 16, 3: 32}      # config -> K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[6, 3])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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
        C, P = R * K, K * (K - 1) // 2
        rng = np.random.default_rng(0xC0000000 + cfg_id)
        raw = synth.make_raw_genotypes(rng, S, K)
        dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
        dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xC0C0 + cfg_id, device=dev)
        torch.cuda.synchronize()
        e = engine.Engine(C, cfg["alphas"], 0.5)
        e.set_genotypes(np.full((S, C, 3), 1.0 / 3.0, dtype=np.float32))
        e.set_pileup_struct(dp.as_struct(), keep=dp)
        e.cluster_stage()
        q = cluster.hwe_prior(np.zeros(S), np.zeros(S))
        e.cluster_mstep(cluster.one_hot_weights(cluster.initial_labels(0, R, B, K), K), q, fetch=False)
        e.set_genotypes_device(e.cluster_device_ptr(), S)
        if dp.pair_snp is None:
            e.set_pileup_struct(dp.as_struct(), keep=dp)
        e.run_singlet()
        log_pi = np.full((R, K), -np.log(K))
        log_delta = np.full(R, np.log(cluster.DELTA0))
        infos = []
        for _ in range(a.warmup + a.reps):
            e.cluster_doublet(R, K)
            e.cluster_estep_doublet(R, K, log_pi, log_delta)
            infos.append(e.cluster_doublet_info())
        e.close()
        timed = infos[a.warmup:]
        dbl = [x["doublet_ms"] for x in timed]
        est = [x["estep_ms"] for x in timed]
        evals = float(dp.n_pairs) * R * P
        med = statistics.median(dbl)
        rec = dict(config=cfg_id, name=cfg["name"], B=B, S=S, K=K, R=R, columns=C, pair_columns=R * P,
                   layout="dense" if dp.pair_snp is None else "sparse", pairs=dp.n_pairs, reads=dp.n_reads, reps=len(timed),
                   doublet_ms=round(med, 3), doublet_ms_min=round(min(dbl), 3), doublet_ms_max=round(max(dbl), 3),
                   estep_ms=round(statistics.median(est), 3), estep_ms_min=round(min(est), 3), estep_ms_max=round(max(est), 3),
                   pair_evaluations=evals, evaluations_per_s=round(evals / (med * 1e-3), -8), lld_bytes=infos[0]["lld_bytes"])
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del dp, dosage
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
