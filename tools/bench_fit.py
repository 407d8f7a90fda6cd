"""Times the goodness-of-fit kernel (k_fit, dmx_engine_fit) at cfg3 (dense, 10k x 50k x 32, GP) and cfg6 (sparse, 20k x 100k x 16,
~2 000 SNPs per barcode): bench.py's panels and device pileups; every barcode as a singlet of its true donor, then every barcode as a
doublet of its true donor and the next one at alpha = 0.5; M = 1, 4, 8.  HIP-event time, median of --reps calls after --warmup.  Beside
each timing, on the same pileup: k_ambient with a one-point grid (Q = 1: the same pairs walked with one log per pair) and the engine's
K1 (run_singlet).  One JSON line per (configuration, kind, M) is appended to --out.

    python tools/bench_fit.py [--configs 3 6] [--reps 10] [--warmup 2] [--out profiles/fit_bench.jsonl]"""
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
    ap.add_argument("--max-reads", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fit_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import bench
    from demuxlet_amd import build, engine, synth, synth_torch
    build.build()
    dev = torch.device("cuda", 0)
    med = lambda xs: round(statistics.median(xs[a.warmup:]), 3)
    for cfg_id in a.configs:
        cfg = bench.CONFIGS[cfg_id]
        B, S, V = cfg["B"], cfg["S"], cfg["V"]
        rng = np.random.default_rng(0xF1700000 + cfg_id)
        raw, g = bench.genotype_matrix(engine, synth, rng, S, V, cfg["field"])
        dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
        dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xF170 + 1000 * cfg_id, device=dev)
        v1 = dp.truth[:, 0].cpu().numpy().astype(np.int32)
        amb = np.clip(raw.alleles, 0, 1).sum(axis=2).mean(axis=1) / 2.0
        torch.cuda.synchronize()
        e = engine.Engine(V, cfg["alphas"], 0.5)
        e.set_genotypes(g)
        e.set_pileup_struct(dp.as_struct(), keep=dp)
        amb_ms, k1_ms = [], []
        for _ in range(a.warmup + a.reps):
            e.ambient_profile(v1, amb, [0.0])
            amb_ms.append(e.ambient_info()["kernel_ms"])
            e.run_singlet(); e.sync()
            k1_ms.append(float(e.kernel_times().singlet_ms))
        hyps = {"singlet": np.stack([v1, np.full(B, -1, dtype=np.int32)], axis=1), "doublet": np.stack([v1, (v1 + 1) % V], axis=1)}
        with open(a.out, "a") as f:
            for kind, hyp in hyps.items():
                for M in a.max_reads:
                    ms, info = [], None
                    for _ in range(a.warmup + a.reps):
                        e.fit_profile(hyp, np.full(B, 0.5), None, None, M)
                        info = e.fit_info()
                        ms.append(info["kernel_ms"])
                    row = dict(config=cfg_id, name=cfg["name"], B=B, S=S, V=V, pairs=dp.n_pairs, reads=dp.n_reads, kind=kind, max_reads=M,
                               reps=a.reps, fit_ms=med(ms), fit_ms_min=round(min(ms[a.warmup:]), 3), fit_ms_max=round(max(ms[a.warmup:]), 3),
                               ambient_q1_ms=med(amb_ms), k1_ms=med(k1_ms), ratio_to_ambient_q1=round(med(ms) / med(amb_ms), 2),
                               n_trunc=info["n_trunc"], n_zero=info["n_zero"])
                    f.write(json.dumps(row) + "\n")
                    print(json.dumps(row), flush=True)
        e.close()
        del dp, dosage
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
