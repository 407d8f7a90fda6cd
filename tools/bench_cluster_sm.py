"""Times the split-merge moves of the genotype-free EM at cfg6 size (sparse, 20k barcodes x 100k SNPs, ~2 000
covered SNPs per barcode, K = 16) and cfg3 size (dense, 10k x 50k, K = 32), R = 4 restarts, on bench.py's device pileups of K donors:
  merge    dmx_engine_cluster_merge_score over the R x K columns of an M-step (k_cluster_marg + k_cluster_merge_part + _fold), HIP events;
  grouped  dmx_engine_cluster_estep_grouped of the sub-EM engine (K x Rs x 2 columns; k_cluster_estep_grp + the ordered sums), HIP events;
  move     one whole move (merge scores, the sub-EM to convergence, the candidates' EM to convergence), wall clock after 5 EM iterations;
  run      cluster_run with and without split_merge=True (wall clock; --run-configs only).
Kernel times are the median of --reps calls after --warmup.  One JSON line per configuration, also appended to --out.

    python tools/bench_cluster_sm.py [--configs 6 3] [--run-configs 6] [--reps 10] [--warmup 2] [--out profiles/cluster_sm_bench.jsonl]"""
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
SHAPES = {6: 16, 3: 32}      # config -> K


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
        B, S, K, R, Rs = cfg["B"], cfg["S"], SHAPES[cfg_id], a.restarts, cluster.SM_SPLIT_RESTARTS
        P = K * (K - 1) // 2
        rng = np.random.default_rng(0xC0000000 + cfg_id)
        raw = synth.make_raw_genotypes(rng, S, K)
        dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
        dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xC0C0 + cfg_id, device=dev)
        z = np.zeros(B, dtype=np.int32)
        pl = engine.HostPileup(rd_totl=z, rd_pass=z, rd_uniq=z, **dp.host_slice(0, B))
        del dp, dosage
        torch.cuda.empty_cache()
        barcodes = [synth.barcode_name(c) for c in range(B)]
        rec = dict(config=cfg_id, B=B, S=S, K=K, R=R, split_restarts=Rs, pairs=int(len(pl.pair_nrd)), layout="dense" if pl.pair_snp is None else "sparse")
        # main engine after a few EM iterations: merge scores, then one whole move from its best restart
        q = cluster.hwe_prior(np.zeros(S), np.zeros(S))
        e = cluster._staged_engine(R * K, pl, S, cfg["alphas"], 0.5, 0, 0)
        try:
            e.cluster_mstep(cluster.one_hot_weights(cluster.initial_labels(0, R, B, K), K), q, fetch=False)
            ll, log_pi, delta, _ = cluster.em_loop(e, pl, S, R, K, q, 1e-3, np.full((R, K), -np.log(K)), np.full(R, cluster.DELTA0), None, B,
                                                   5, 1e-7, 1.0, False)
            ms = []
            for _ in range(a.warmup + a.reps):
                e.cluster_merge_score(R, K, q)
                ms.append(e.cluster_sm_info()["merge_ms"])
            rec["merge_ms"] = statistics.median(ms[a.warmup:])
            rec["merge_terms"] = R * P * S
            win = cluster.best_restart(ll)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, rows = cluster.split_merge_moves(e, win, R, float(ll[win]), float(delta[win]), pl, S, K, q, 1e-3, None, B, 50, 1e-7, 1.0, False,
                                                0, 1, cluster.SM_CANDIDATES, Rs, cfg["alphas"], 0.5, 0, 0)
            rec["move_s"] = time.perf_counter() - t0
            rec["move_candidates"] = len(rows)
            rec["move_candidate_iterations"] = rows[0]["iterations"] if rows else 0
        finally:
            e.close()
        # the sub-EM engine: grouped E-step
        s = cluster._staged_engine(K * Rs * 2, pl, S, cfg["alphas"], 0.5, 0, 0)
        try:
            group = (np.arange(B) % K).astype(np.int32)
            s.cluster_mstep(cluster.sub_restart_weights(group, K, Rs, 0), q, fetch=False)
            s.set_genotypes_device(s.cluster_device_ptr(), S)
            if pl.pair_snp is None:
                s.set_pileup(pl)
            t0 = time.perf_counter()
            s.run_singlet()
            s.sync()
            rec["sub_k1_wall_ms"] = 1e3 * (time.perf_counter() - t0)
            gs = []
            for _ in range(a.warmup + a.reps):
                s.cluster_estep_grouped(K * Rs, 2, np.full((K * Rs, 2), -np.log(2.0)), group, Rs)
                gs.append(s.cluster_sm_info()["grouped_estep_ms"])
            rec["grouped_estep_ms"] = statistics.median(gs[a.warmup:])
        finally:
            s.close()
        if cfg_id in a.run_configs:
            with tempfile.TemporaryDirectory() as d:
                for sm in (False, True):
                    t0 = time.perf_counter()
                    res = cluster.cluster_run(pl, K, str(Path(d) / "o"), restarts=R, seed=1, barcodes=barcodes, split_merge=sm)
                    key = "run_sm" if sm else "run_plain"
                    rec[key + "_s"] = time.perf_counter() - t0
                    if sm:
                        rec["run_sm_candidates"] = len(res["moves"])
                        rec["run_sm_accepted"] = sum(int(r["accepted"]) for r in res["moves"])
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
