"""Times the parts that choose the number of clusters at cfg6 size (sparse, 20k barcodes x 100k SNPs, ~2 000
covered SNPs per barcode, K_true = 16) and cfg3 size (dense, 10k x 50k, K_true = 32), R = 4 restarts of K_max = 2 K_true columns, on
bench.py's device pileups of K_true donors, after 5 EM iterations:
  evidence  dmx_engine_cluster_evidence over the R x K_max columns of an M-step (k_cluster_marg + k_cluster_ev_part + _fold);
  hard      dmx_engine_cluster_hard on the last E-step's weights (k_cluster_hard + k_cluster_hard_part + _fold);
  merge_columns  dmx_engine_cluster_merge_columns (k_cluster_merge_cols);
  mstep, merge   the M-step on the one-hot matrix and dmx_engine_cluster_merge_score on it, in the same process, for comparison;
  run       cluster_run(auto_k=True) at K_max beside the fixed-K run at K_true on the same data, plain and with em_doublets=True
            (wall clock; --run-configs only).
Kernel times are HIP events, the median of --reps calls after --warmup.  One JSON line per configuration, also appended to --out.

    python tools/bench_cluster_k.py [--configs 6 3] [--run-configs 6] [--reps 10] [--warmup 2] [--out profiles/cluster_k_bench.jsonl]"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SHAPES = {6: 16, 3: 32}      # config -> K_true


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[6, 3])
    ap.add_argument("--run-configs", type=int, nargs="*", default=[6])
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
        B, S, Kt, R = cfg["B"], cfg["S"], SHAPES[cfg_id], a.restarts
        K = 2 * Kt
        rng = np.random.default_rng(0xC0000000 + cfg_id)
        raw = synth.make_raw_genotypes(rng, S, Kt)
        dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
        dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xC0C0 + cfg_id, device=dev)
        z = np.zeros(B, dtype=np.int32)
        pl = engine.HostPileup(rd_totl=z, rd_pass=z, rd_uniq=z, **dp.host_slice(0, B))
        del dp, dosage
        torch.cuda.empty_cache()
        barcodes = [synth.barcode_name(c) for c in range(B)]
        rec = dict(config=cfg_id, B=B, S=S, K_true=Kt, K_max=K, R=R, pairs=int(len(pl.pair_nrd)), layout="dense" if pl.pair_snp is None else "sparse")
        q = cluster.hwe_prior(np.zeros(S), np.zeros(S))
        e = cluster._staged_engine(R * K, pl, S, cfg["alphas"], 0.5, 0, 0)
        try:
            e.cluster_mstep(cluster.one_hot_weights(cluster.initial_labels(0, R, B, K), K), q, fetch=False)
            cluster.em_loop(e, pl, S, R, K, q, 1e-3, np.full((R, K), -np.log(K)), np.full(R, cluster.DELTA0), None, B, 5, 1e-7, 1.0, False)
            active = np.ones((R, K), dtype=np.uint8)
            t = dict(hard=[], mstep=[], evidence=[], merge=[], merge_columns=[])
            for i in range(a.warmup + a.reps):
                e.cluster_hard(R, K, active)
                t["hard"].append(e.cluster_k_info()["hard_ms"])
                e.cluster_mstep(e.cluster_hard_device_ptr(), q, fetch=False)
                t["mstep"].append(e.cluster_info()["mstep_ms"])
                e.cluster_evidence(R, K, q)
                t["evidence"].append(e.cluster_k_info()["evidence_ms"])
                e.cluster_merge_score(R, K, q)
                t["merge"].append(e.cluster_sm_info()["merge_ms"])
                # (columns 2 i and 2 i + 1: a fresh pair every call, so the merged column is never already empty)
                e.cluster_merge_columns(R, K, np.full(R, 2 * i + 1, dtype=np.int32), np.full(R, 2 * i, dtype=np.int32))
                t["merge_columns"].append(e.cluster_k_info()["merge_columns_ms"])
            for k, v in t.items():
                rec[k + "_ms"] = statistics.median(v[a.warmup:])
            rec["evidence_plus_hard_over_mstep"] = (rec["evidence_ms"] + rec["hard_ms"]) / rec["mstep_ms"]
        finally:
            e.close()
        if cfg_id in a.run_configs:
            # plain EM, then with doublet components (the bench's pools hold doublets, which plain EM keeps as clusters of their own)
            with tempfile.TemporaryDirectory() as d:
                for dbl, tag in ((False, ""), (True, "_dbl")):
                    t0 = time.perf_counter()
                    res = cluster.cluster_run(pl, Kt, str(Path(d) / "f"), restarts=R, seed=1, barcodes=barcodes, em_doublets=dbl)
                    rec[f"run_fixed{tag}_s"], rec[f"run_fixed{tag}_iterations"] = time.perf_counter() - t0, int(res["iterations"])
                    t0 = time.perf_counter()
                    res = cluster.cluster_run(pl, K, str(Path(d) / "a"), restarts=R, seed=1, barcodes=barcodes, auto_k=True, em_doublets=dbl)
                    rec[f"run_auto{tag}_s"] = time.perf_counter() - t0
                    rec[f"run_auto{tag}_k"] = int(res["n_clusters"])
                    rec[f"run_auto{tag}_iterations"] = int(open(str(Path(d) / "a.em.tsv")).read().splitlines()[-1].split("\t")[0])
                    rec[f"run_auto{tag}_steps"] = len(res["kpath"]) // R
                    rec[f"run_auto{tag}_best_score_by_k"] = {str(k): round(max(r["score"] for r in res["kpath"] if r["k"] == k), 1)
                                                             for k in sorted({r["k"] for r in res["kpath"]}, reverse=True)}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
