"""Times the pileup composer (dmx_engine_compose: k_compose<count>, k_compose_scan, k_compose<fill>) at the cfg6 shape (sparse, 20k x 100k x 16,
~2 000 SNPs per barcode): 20 000 HET rows (two parents of different donors, share 0.5) at depth F = 1 (every read kept) and F = 0.25.
HIP-event times, the median of 5 runs after a warm-up; algorithmic bytes from dmx_engine_compose_info; GB/s over the sum of the three
kernels and its share of the achievable HBM rate (6.3 TB/s).  The numpy restatement (tests/compose_ref.py) is timed on a recipe
of its own (--ref-rows HET rows over the first cells, at the same thresholds) and scaled to the full recipe, so that the record shows a
ratio; the timed recipe draws its parents uniformly from the whole pool.  Prints one JSON line per depth and appends it to
profiles/compose_bench.jsonl.

    python tools/bench_compose.py [--rows 20000] [--ref-rows 1000] [--no-append]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
HBM_GBS = 6300.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--ref-rows", type=int, default=1000)
    ap.add_argument("--no-append", action="store_true")
    a = ap.parse_args()
    import torch
    import bench
    import compose_ref
    from demuxlet_amd import build, engine, simulate, synth, synth_torch
    build.build()
    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[6]
    B, S, V = cfg["B"], cfg["S"], cfg["V"]
    rng = np.random.default_rng(0xC0350000)
    raw, g = bench.genotype_matrix(engine, synth, rng, S, V, cfg["field"])
    dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
    dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0xC035, device=dev)
    donor = dp.truth[:, 0].cpu().numpy()
    def het_rows(n, cells):
        par = np.zeros((n, 2), dtype=np.int32)
        for k in range(n):
            p = int(rng.integers(cells)); q = int(rng.integers(cells))
            while donor[q] == donor[p]:
                q = int(rng.integers(cells))
            par[k] = (p, q)
        return par

    # the timed recipe draws its parents from the whole pool; the restatement gets a recipe of its own over the first cells, the slice
    # that is copied to the host, and the GPU composes that recipe once, untimed, to show that both made the same barcodes
    par = het_rows(a.rows, B)
    n_ref = min(a.ref_rows, a.rows)
    ref_cells = min(B, max(2 * V, 2 * n_ref))
    ref_par = het_rows(n_ref, ref_cells)
    hs = SimpleNamespace(**dp.host_slice(0, ref_cells))
    torch.cuda.synchronize()
    e = engine.Engine(V, cfg["alphas"], 0.5)
    e.set_genotypes(g)
    e.set_pileup_struct(dp.as_struct(), keep=dp)
    for depth in (1.0, 0.25):
        thr = simulate.threshold(2.0 * 0.5 * depth)
        keep = np.full((a.rows, 2), thr, dtype=np.uint64)
        runs = []
        for i in range(6):
            runs.append(e.compose(par, keep, 0xBE7C))
        runs = runs[1:]
        inf = runs[-1]
        med = {k: statistics.median(r[k] for r in runs) for k in ("count_ms", "scan_ms", "fill_ms")}
        tot = [r["count_ms"] + r["scan_ms"] + r["fill_ms"] for r in runs]
        ms = statistics.median(tot)
        nbytes = inf["bytes_read"] + inf["bytes_written"]
        gbs = nbytes / (ms * 1e-3) / 1e9
        t0 = time.perf_counter()
        ref = compose_ref.compose(hs, ref_par, keep[:n_ref], 0xBE7C)
        ref_s = time.perf_counter() - t0
        e.compose(ref_par, keep[:n_ref], 0xBE7C)
        got = e.get_composed()
        assert np.array_equal(ref["cell_pair_off"], got.cell_pair_off) and np.array_equal(ref["pair_snp"], got.pair_snp)
        assert np.array_equal(ref["pair_nrd"], got.pair_nrd) and np.array_equal(ref["reads"], got.reads)
        ref_full_ms = ref_s * 1e3 * a.rows / n_ref
        row = dict(config=6, B=B, S=S, V=V, src_pairs=dp.n_pairs, src_reads=dp.n_reads, rows=a.rows, kind="HET", depth=depth, reps=len(runs),
                   compose_ms=round(ms, 3), compose_ms_min=round(min(tot), 3), compose_ms_max=round(max(tot), 3),
                   count_ms=round(med["count_ms"], 3), scan_ms=round(med["scan_ms"], 3), fill_ms=round(med["fill_ms"], 3),
                   out_pairs=inf["n_pairs"], out_reads=inf["n_reads"], nrd_width=inf["nrd_width"], bytes_read=inf["bytes_read"],
                   bytes_written=inf["bytes_written"], gb_per_s=round(gbs, 1), hbm_share=round(gbs / HBM_GBS, 4),
                   numpy_rows=n_ref, numpy_s=round(ref_s, 3), numpy_full_ms=round(ref_full_ms, 1), numpy_over_gpu=round(ref_full_ms / ms, 1))
        line = json.dumps(row)
        print(line, flush=True)
        if not a.no_append:
            with open(ROOT / "profiles" / "compose_bench.jsonl", "a") as f:
                f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
