"""Times the site audit (k_site_partial + k_site_fold, dmx_engine_site_fit) at cfg3 (dense, 10k x 50k x 32, GP) and cfg6 (sparse,
20k x 100k x 16, ~2 000 SNPs per barcode): bench.py's panels and device pileups; every barcode as a singlet of its true donor, then every
barcode as a doublet of its true donor and the next one at alpha = 0.5; M = 1, 4, 8.  HIP-event time, median of --reps calls after
--warmup.  Beside each timing, on the same pileup and hypotheses: k_fit (dmx_engine_fit: the same per-pair work without the per-SNP
reduction) and k_refine_partial + k_refine_fold (dmx_engine_refine_genotypes with every barcode assigned to its true donor: the same
reduction scheme with three logs per pair).  One JSON line per (configuration, kind, M) is appended to --out.

    python tools/bench_sites.py [--configs 3 6] [--reps 10] [--warmup 2] [--out profiles/sites_bench.jsonl]"""
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sites_bench.jsonl"))
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
        torch.cuda.synchronize()
        e = engine.Engine(V, cfg["alphas"], 0.5)
        e.set_genotypes(g)
        e.set_pileup_struct(dp.as_struct(), keep=dp)
        ref_ms = []
        for _ in range(a.warmup + a.reps):
            e.refine_genotypes(v1, g)
            ref_ms.append(e.refine_info()["partial_ms"])
        hyps = {"singlet": np.stack([v1, np.full(B, -1, dtype=np.int32)], axis=1), "doublet": np.stack([v1, (v1 + 1) % V], axis=1)}
        slabs = -(-S // 512)
        with open(a.out, "a") as f:
            for kind, hyp in hyps.items():
                for M in a.max_reads:
                    ms, fit_ms, info = [], [], None
                    for _ in range(a.warmup + a.reps):
                        e.site_fit(hyp, np.full(B, 0.5), None, None, M)
                        info = e.site_fit_info()
                        ms.append(info["kernel_ms"])
                        e.fit_profile(hyp, np.full(B, 0.5), None, None, M)
                        fit_ms.append(e.fit_info()["kernel_ms"])
                    row = dict(config=cfg_id, name=cfg["name"], B=B, S=S, V=V, pairs=dp.n_pairs, reads=dp.n_reads, kind=kind, max_reads=M,
                               reps=a.reps, site_ms=med(ms), site_ms_min=round(min(ms[a.warmup:]), 3), site_ms_max=round(max(ms[a.warmup:]), 3),
                               fit_ms=med(fit_ms), refine_partial_fold_ms=med(ref_ms), ratio_to_fit=round(med(ms) / med(fit_ms), 2),
                               ratio_to_refine=round(med(ms) / med(ref_ms), 2), pairs_per_barcode_slab=round(dp.n_pairs / B / slabs, 1),
                               n_chunks=info["n_chunks"], n_waves=info["n_waves"], partial_bytes=info["partial_bytes"], slab_snps=info["slab_snps"],
                               n_trunc=info["n_trunc"], n_zero=info["n_zero"])
                    f.write(json.dumps(row) + "\n")
                    print(json.dumps(row), flush=True)
        e.close()
        del dp, dosage
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
