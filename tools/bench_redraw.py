"""Times the model-drawn null pool (k_redraw, dmx_engine_redraw) at cfg6 (sparse, 20k x 100k x 16, ~2 000 SNPs per barcode) and cfg3
(dense, 10k x 50k x 32, GP): bench.py's panels and device pileups; every barcode as a singlet of its true donor, then every barcode as a
doublet of its true donor and the next one at alpha = 0.5; both draw modes.  The kernel's HIP-event time (dmx_redraw_info.kernel_ms: the
whole-array copy that precedes the kernel is not in it), median of --reps calls after --warmup.  Beside it, on the same device, a
device-to-device copy of the same `reads` bytes (torch, HIP events) — the floor of any pass that reads and writes every read byte once —
and the pileup composer's GB/s from profiles/compose_bench.jsonl (its depth-1 row) for comparison.  One JSON line per (configuration,
kind, draw) is appended to --out.

    python tools/bench_redraw.py [--configs 6 3] [--reps 10] [--warmup 2] [--out profiles/redraw_bench.jsonl]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HBM_GB_PER_S = 6300.0                              # the rate profiles/compose_bench.jsonl's hbm_share is taken against


def compose_reference():
    path = ROOT / "profiles" / "compose_bench.jsonl"
    if not path.exists():
        return None
    rows = [json.loads(l) for l in path.read_text().splitlines() if l.strip()]
    full = [r for r in rows if r.get("depth") == 1.0]
    return dict(gb_per_s=full[0]["gb_per_s"], hbm_share=full[0]["hbm_share"]) if full else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[6, 3])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "redraw_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import bench
    from demuxlet_amd import build, engine, synth, synth_torch
    build.build()
    dev = torch.device("cuda", 0)
    med = lambda xs: statistics.median(xs[a.warmup:])
    cmp_ref = compose_reference()
    for cfg_id in a.configs:
        cfg = bench.CONFIGS[cfg_id]
        B, S, V = cfg["B"], cfg["S"], cfg["V"]
        rng = np.random.default_rng(0x4ED40000 + cfg_id)
        raw, g = bench.genotype_matrix(engine, synth, rng, S, V, cfg["field"])
        dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
        dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0x4ED4 + 1000 * cfg_id, device=dev)
        v1 = dp.truth[:, 0].cpu().numpy().astype(np.int32)
        src = torch.empty(dp.n_reads, dtype=torch.uint8, device=dev).random_(0, 256)
        dst = torch.empty_like(src)
        copy_ms = []
        for _ in range(a.warmup + a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); dst.copy_(src); t1.record()
            torch.cuda.synchronize()
            copy_ms.append(t0.elapsed_time(t1))
        del src, dst
        e = engine.Engine(V, cfg["alphas"], 0.5)
        e.set_genotypes(g)
        e.set_pileup_struct(dp.as_struct(), keep=dp)
        hyps = {"singlet": np.stack([v1, np.full(B, -1, dtype=np.int32)], axis=1), "doublet": np.stack([v1, (v1 + 1) % V], axis=1)}
        with open(a.out, "a") as f:
            for kind, hyp in hyps.items():
                for draw in ("donor", "pair"):
                    ms, info = [], None
                    for k in range(a.warmup + a.reps):
                        info = e.redraw(hyp, np.full(B, 0.5), None, None, seed=1, geno_seed=2, genotype_draw=draw, index_base=k * B)
                        ms.append(info["kernel_ms"])
                    t = med(ms)
                    gbs = (info["bytes_read"] + info["bytes_written"]) / t / 1e6
                    row = dict(config=cfg_id, name=cfg["name"], B=B, S=S, V=V, pairs=dp.n_pairs, reads=dp.n_reads, kind=kind, draw=draw, reps=a.reps,
                               kernel_ms=round(t, 3), kernel_ms_min=round(min(ms[a.warmup:]), 3), kernel_ms_max=round(max(ms[a.warmup:]), 3),
                               bytes_read=info["bytes_read"], bytes_written=info["bytes_written"], gb_per_s=round(gbs, 1),
                               hbm_share=round(gbs / HBM_GB_PER_S, 4), n_pairs_drawn=info["n_pairs_drawn"], n_pairs_skipped=info["n_pairs_skipped"],
                               n_reads_drawn=info["n_reads_drawn"], n_reads_kept=info["n_reads_kept"],
                               reads_copy_ms=round(med(copy_ms), 3), reads_copy_gb_per_s=round(2 * dp.n_reads / med(copy_ms) / 1e6, 1),
                               kernel_over_copy=round(t / med(copy_ms), 2),
                               compose_gb_per_s=cmp_ref["gb_per_s"] if cmp_ref else None, compose_hbm_share=cmp_ref["hbm_share"] if cmp_ref else None)
                    f.write(json.dumps(row) + "\n")
                    print(json.dumps(row), flush=True)
        e.close()
        del dp, dosage
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
