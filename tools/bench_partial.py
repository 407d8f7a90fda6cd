"""Times the EM of partly genotyped pools at cfg6 size (sparse, 20k barcodes x 100k SNPs, ~2 000 covered SNPs per
barcode): bench.py's device pileup of 16 donors, 12 known and M = 4 unknown, R = 8 restarts.
  shared   the layout of demuxlet_amd.partial: V = Vk + R M columns (44); per iteration K1's HIP-event time, cluster_estep_known's and
           cluster_mstep_window's (dmx_engine_cluster_known_info);
  naive    R restarts x (Vk + M) columns (128) through the plain cluster_estep / cluster_mstep, the known columns repeated per restart;
  start    (--runs) partial_run end to end from the seeded start (known donors' barcodes on their donor) and from a plain random start
           (every barcode on a random free column): iterations, wall clock, the dropped donors' and the known donors' singlets called
           right.
Kernel times are the medians of iterations 2 .. --iters.  One JSON line per leg, also appended to --out.

    python tools/bench_partial.py [--iters 6] [--runs] [--out profiles/partial_bench.jsonl]"""
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
V_ALL, VK, M, R = 16, 12, 4, 8
DROPPED = [3, 8, 12, 15]


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def med(its, key):
    return round(statistics.median(x[key] for x in its[1:] or its), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--runs", action="store_true", help="also partial_run end to end, seeded against random start")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from demuxlet_amd import build, cluster, engine, partial, synth, synth_torch
    build.build()
    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[6]
    B, S = cfg["B"], cfg["S"]
    rng = np.random.default_rng(0xC0000006)
    raw = synth.make_raw_genotypes(rng, S, V_ALL)
    dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
    dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xC0C6, device=dev)
    torch.cuda.synchronize()
    known = [v for v in range(V_ALL) if v not in DROPPED]
    g = engine.geno_from_gt(raw.alleles, 0.01).reshape(S, V_ALL, 3)
    gk = np.ascontiguousarray(g[:, known])
    q = cluster.hwe_prior(np.zeros(S), np.zeros(S))
    base = dict(config=6, B=B, S=S, known=VK, unknown=M, R=R, pairs=dp.n_pairs)

    # shared layout: [known | R x M]
    V = VK + R * M
    e = engine.Engine(V, cfg["alphas"], 0.5)
    try:
        e.set_genotypes(np.full((S, V, 3), 1.0 / 3.0, dtype=np.float32))
        e.set_pileup_struct(dp.as_struct(), keep=dp)
        e.cluster_stage()
        e.cluster_set_known(gk)
        lab = partial.random_labels(0, R, B, VK, M)
        e.cluster_mstep_window(partial.free_weights(lab, VK, M), R, M, q, fetch=False)
        log_pi = np.full((R, VK + M), -np.log(VK + M))
        its = []
        for _ in range(a.iters):
            t1 = time.perf_counter()
            e.set_genotypes_device(e.cluster_device_ptr(), S)
            e.run_singlet()
            k1 = e.kernel_times().singlet_ms
            ll, cs = e.cluster_estep_known(R, VK, M, log_pi)
            log_pi = cluster.update_log_pi(cs, R, VK + M)
            e.cluster_mstep_window(None, R, M, q, fetch=False)
            inf = e.cluster_known_info()
            its.append(dict(k1_ms=k1, estep_ms=inf["estep_ms"], mstep_ms=inf["mstep_ms"], wall_ms=1e3 * (time.perf_counter() - t1)))
    finally:
        e.close()
    emit(dict(base, leg="shared", columns=V, k1_ms_median=med(its, "k1_ms"), estep_ms_median=med(its, "estep_ms"),
              mstep_ms_median=med(its, "mstep_ms"), iteration_wall_ms_median=med(its, "wall_ms"),
              per_iteration=[{k: round(v, 3) for k, v in x.items()} for x in its]), a.out)

    # naive layout: R restarts x (Vk + M) columns, the known columns in every restart
    K = VK + M
    C = R * K
    e = engine.Engine(C, cfg["alphas"], 0.5)
    try:
        e.set_genotypes(np.full((S, C, 3), 1.0 / 3.0, dtype=np.float32))
        e.set_pileup_struct(dp.as_struct(), keep=dp)
        e.cluster_stage()
        e.cluster_mstep(cluster.one_hot_weights(cluster.initial_labels(0, R, B, K), K), q, fetch=False)
        log_pi = np.full((R, K), -np.log(K))
        its = []
        for _ in range(a.iters):
            t1 = time.perf_counter()
            e.set_genotypes_device(e.cluster_device_ptr(), S)
            e.run_singlet()
            k1 = e.kernel_times().singlet_ms
            ll, cs = e.cluster_estep(R, K, log_pi)
            log_pi = cluster.update_log_pi(cs, R, K)
            e.cluster_mstep(None, q, fetch=False)
            inf = e.cluster_info()
            its.append(dict(k1_ms=k1, estep_ms=inf["estep_ms"], mstep_ms=inf["mstep_ms"], wall_ms=1e3 * (time.perf_counter() - t1)))
    finally:
        e.close()
    emit(dict(base, leg="naive", columns=C, k1_ms_median=med(its, "k1_ms"), estep_ms_median=med(its, "estep_ms"),
              mstep_ms_median=med(its, "mstep_ms"), iteration_wall_ms_median=med(its, "wall_ms"),
              per_iteration=[{k: round(v, 3) for k, v in x.items()} for x in its]), a.out)

    if a.runs:
        h = dp.host_slice(0, B)
        truth = dp.truth.cpu().numpy()
        z = np.zeros(B, dtype=np.int32)
        pl = engine.HostPileup(rd_totl=z, rd_pass=z, rd_uniq=z, **h)
        barcodes = [synth.barcode_name(c) for c in range(B)]
        ids = [f"donor{v}" for v in known]
        singlet = truth[:, 1] < 0
        for start in ("seeded", "random"):
            init = None if start == "seeded" else partial.random_labels(1, R, B, VK, M)
            with tempfile.TemporaryDirectory() as d:
                t0 = time.perf_counter()
                res = partial.partial_run(pl, gk, ids, M, str(Path(d) / "p"), restarts=R, seed=1, barcodes=barcodes, init_labels=init)
                wall = time.perf_counter() - t0
                best = {}
                with open(str(Path(d) / "p.best")) as f:
                    head = f.readline().rstrip("\n").split("\t")
                    col = {n: i for i, n in enumerate(head)}
                    for ln in f:
                        t = ln.rstrip("\n").split("\t")
                        best[t[col["BARCODE"]]] = t[col["BEST"]]
            calls = [best.get(b, "") for b in barcodes]
            kc = np.array([known[ids.index(c[4:])] if c.startswith("SNG-donor") else -1 for c in calls])
            uc = np.array([int(c[7:]) if c.startswith("SNG-UNK") else -1 for c in calls])
            tu = np.where(singlet & np.isin(truth[:, 0], DROPPED), np.searchsorted(DROPPED, truth[:, 0]), -1)
            lab = cluster.match_labels(tu, uc, len(DROPPED), M)
            mapped = np.where(uc >= 0, lab[np.maximum(uc, 0)], -1)
            ks = singlet & np.isin(truth[:, 0], known)
            emit(dict(base, leg=f"run_{start}", iterations=res["iterations"], restart=res["restart"], wall_s=round(wall, 3),
                      ll_best=float(np.max(res["ll"])), ll_restarts=[round(float(x), 3) for x in res["ll"]],
                      unknown_singlets_right=round(float((mapped[tu >= 0] == tu[tu >= 0]).mean()), 4),
                      known_singlets_right=round(float((kc[ks] == truth[ks, 0]).mean()), 4),
                      doublets_dbl=round(float(np.mean([c.startswith("DBL-") for c, s in zip(calls, singlet) if not s])), 4)), a.out)
    del dp, dosage
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
