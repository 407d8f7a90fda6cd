"""Times the continuous mixing share (dmx_engine_share_scan / _share_fit) at cfg6 (sparse, 20k x 100k x 16,
~2 000 SNPs per barcode) and cfg3 (dense, 10k x 50k x 32, GP) with T = 1 anchor (the true first donor) and C = 5 candidates (the four
partners of highest z and the pair (truth, truth + 1)).  HIP-event times, median of --reps calls after --warmup:

  scan_ms, fit_ms      k_share_scan, k_share_fit (tol 1e-6, start 0.5, no probe), and the evaluations per candidate the fit ran
  ambient_dbl_ms       k_ambient_dbl at A = 1, Q = 1 (alpha 0.5, rho 0) over the same candidates, timed beside them: one evaluation of
                       LL alone by the existing kernel
  strict_ms            the engine's own STRICT doublet step (K2) at --alpha 0 0.5 and at 0 0.1 0.2 0.3 0.4 0.5: the finer grid is
                       the price of the same sensitivity today

One JSON line per configuration, appended to profiles/share_bench.jsonl.

    python tools/bench_share.py [--configs 6 3] [--reps 10] [--warmup 2]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

FINE = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[6, 3])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "share_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import bench
    from demuxlet_amd import build, engine, share, synth, synth_torch
    build.build()
    dev = torch.device("cuda", 0)
    med = statistics.median
    for cfg_id in a.configs:
        cfg = bench.CONFIGS[cfg_id]
        B, S, V = cfg["B"], cfg["S"], cfg["V"]
        rng = np.random.default_rng(0xD3A00000 + cfg_id)
        raw, g = bench.genotype_matrix(engine, synth, rng, S, V, cfg["field"])
        dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
        dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xD3A0 + 1000 * cfg_id, device=dev)
        t0 = dp.truth[:, 0].cpu().numpy().astype(np.int32)
        zeros = np.zeros(S)
        torch.cuda.synchronize()
        strict = {}
        for name, alphas in (("coarse", (0.0, 0.5)), ("fine", FINE)):
            e = engine.Engine(V, alphas, 0.5)
            e.set_genotypes(g)
            e.set_pileup_struct(dp.as_struct(), keep=dp)
            ts = []
            for i in range(a.warmup + a.reps):
                e.run()
                e.sync()
                ts.append(float(e.kernel_times().doublet_ms))
            strict[name] = ts[a.warmup:]
            e.close()
        e = engine.Engine(V, (0.0, 0.5), 0.5)
        e.set_genotypes(g)
        e.set_pileup_struct(dp.as_struct(), keep=dp)
        anchors = t0[:, None].copy()
        d_anc = torch.from_numpy(anchors).to(dev)
        scan, _, _ = e.share_scan(int(d_anc.data_ptr()), n_anchor=1)
        cand, _ = share.select_candidates(scan, anchors, 4, t0, (t0 + 1) % V)
        d_cand = torch.from_numpy(cand).to(dev)
        sc, ft, ad, evals = [], [], [], 0.0
        for i in range(a.warmup + a.reps):
            e.share_scan(int(d_anc.data_ptr()), n_anchor=1)
            sc.append(e.share_info()["scan_ms"])
            f = e.share_fit(int(d_cand.data_ptr()), n_cand=5)
            inf = e.share_info()
            ft.append(inf["fit_ms"])
            evals = inf["fit_evals"] / max(inf["fit_used"], 1)
            e.ambient_doublet_profile(int(d_cand.data_ptr()), [0.5], zeros, [0.0], n_cand=5)
            ad.append(e.ambient_doublet_info()["kernel_ms"])
        sc, ft, ad = sc[a.warmup:], ft[a.warmup:], ad[a.warmup:]
        used = int((cand[:, :, 0] >= 0).sum())
        interior = int(((f["status"] & 1) != 0).sum())
        rec = dict(config=cfg_id, B=B, S=S, V=V, pairs=dp.n_pairs, reads=dp.n_reads, n_anchor=1, n_cand=5, reps=len(sc), cand_used=used,
                   cand_interior=interior, evals_per_cand=round(evals, 3),
                   scan_ms=round(med(sc), 3), scan_ms_min=round(min(sc), 3), scan_ms_max=round(max(sc), 3),
                   fit_ms=round(med(ft), 3), fit_ms_min=round(min(ft), 3), fit_ms_max=round(max(ft), 3),
                   fit_ms_per_eval=round(med(ft) / max(evals, 1e-9), 3),
                   ambient_dbl_ms=round(med(ad), 3), ambient_dbl_ms_min=round(min(ad), 3), ambient_dbl_ms_max=round(max(ad), 3),
                   strict_ms_alpha_0_05=round(med(strict["coarse"]), 3), strict_ms_alpha_6=round(med(strict["fine"]), 3),
                   strict_extra_ms=round(med(strict["fine"]) - med(strict["coarse"]), 3),
                   share_pass_ms=round(med(sc) + med(ft), 3))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
        e.close()
        del dp, dosage
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
