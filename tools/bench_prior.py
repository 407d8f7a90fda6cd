"""Times the empirical-Bayes prior pass (dmx_engine_prior_step / _fit / _call) on grids of cfg3's size (10 000
barcodes x 32 x 32 x 2 doubles = 164 MB) and cfg6's (20 000 x 16 x 16 x 2 = 82 MB, which fits the Infinity Cache), generated on the
device from a seed: every barcode a singlet or a pair drawn from uneven shares, the true entries standing above the rest.

Per size: the HIP-event times of one iteration's E-step (k_prior_estep) and fold (k_prior_rank + k_prior_fold_chunk + k_prior_fold), median of
--reps calls after --warmup; the achieved GB/s of the E-step over the grid's bytes (the pass reads the grid once from memory and
writes B (V + 3) doubles) beside a device-to-device copy of the same bytes timed in the same run with events (a copy reads and writes
them, so it moves twice the bytes: both figures are given); the record kernel; and a whole fit at tol 1e-6 with its wall time.

Then the quality table: a synth.make_pool_pileup pool (8 donors with shares 0.4 .. 0.03 and one absent, a fifth of the droplets holding
two cells) at about 30 and about 300 SNPs per barcode through prior.prior_run: the largest share error, d against the drawn rate, and
the fraction of right calls of BEST (the reference's) and CALL (under the fitted priors) against truth, where a homotypic doublet
counts as its singlet.

Prints one JSON line per measurement and appends it to profiles/prior_bench.jsonl.

    python tools/bench_prior.py [--reps 10] [--warmup 2] [--no-quality] [--out profiles/prior_bench.jsonl]"""
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

SIZES = {"cfg3": dict(B=10000, V=32, A=2), "cfg6": dict(B=20000, V=16, A=2)}
POOL_SHARES = (0.40, 0.20, 0.15, 0.10, 0.07, 0.05, 0.03, 0.0)


def device_grid(torch, dev, B, V, A, seed):
    """[B][V][V][A] float64 on the device: noise below -30, the true singlet (or pair) 30 above it."""
    gen = torch.Generator(device=dev); gen.manual_seed(seed)
    g = -30.0 - 30.0 * torch.rand((B, V, V, A), generator=gen, device=dev, dtype=torch.float64)
    shares = torch.tensor([1.0 / (1 + j) for j in range(V)], device=dev, dtype=torch.float64)
    first = torch.multinomial(shares, B, replacement=True, generator=gen)
    second = torch.multinomial(shares, B, replacement=True, generator=gen)
    dbl = (torch.rand(B, generator=gen, device=dev) < 0.15) & (first != second)
    b = torch.arange(B, device=dev)
    g[b, first, 0, 0] += 15.0 + 15.0 * (~dbl).to(torch.float64)
    bd = b[dbl]
    g[bd, second[dbl], 0, 0] += 15.0
    for n in range(1, A):
        g[bd, first[dbl], second[dbl], n] += 30.0
        g[bd, second[dbl], first[dbl], n] += 30.0
    return g


def quality(engine, prior, synth, out, snps_per_barcode, emit):
    V, S, B = len(POOL_SHARES), 3000, 3000
    rng = np.random.default_rng(0xEB000 + snps_per_barcode)
    raw = synth.make_raw_genotypes(rng, S, V)
    sp, truth = synth.make_pool_pileup(rng, raw.alleles, B, snps_per_barcode / S, 1.5, POOL_SHARES, 0.2)
    g = engine.geno_from_gt(raw.alleles, 0.01).reshape(S, V, 3)
    pl = engine.HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads, sp.rd_totl, sp.rd_pass,
                           sp.rd_uniq)
    sms = [f"s{j}" for j in range(V)]
    bcs = [synth.barcode_name(i) for i in range(B)]
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        r = prior.prior_run(pl, g, sms, str(Path(d) / "q"), barcodes=bcs)
        wall = time.perf_counter() - t0
        eb = [x.split("\t") for x in (Path(d) / "q.eb.tsv").read_text().splitlines()][1:]
    f = r["fit"]
    right = {"BEST": 0, "CALL": 0}
    sng_as_dbl = {"BEST": 0, "CALL": 0}
    het_found = {"BEST": 0, "CALL": 0}
    n_sng = n_het = 0
    for row, k in zip(eb, r["order"]):
        a, b = int(truth["first"][k]), int(truth["second"][k])
        het = b >= 0 and b != a
        n_het += het; n_sng += not het
        want = ("DBL", frozenset((sms[a], sms[b]))) if het else ("SNG", frozenset((sms[a],)))
        for col, name in ((2, "BEST"), (3, "CALL")):
            t = row[col].split("-")
            got = (t[0], frozenset(t[1:3]) if t[0] == "DBL" else frozenset(t[1:2]))
            right[name] += got == want
            sng_as_dbl[name] += (not het) and t[0] == "DBL"
            het_found[name] += het and t[0] == "DBL"
    n = len(eb)
    emit(what="quality", snps_per_barcode=round(float(np.diff(sp.cell_pair_off).mean()), 1), B=B, V=V, barcodes_called=n, n_iter=f["n_iter"],
         converged=bool(f["converged"]), share_err_max=float(np.abs(f["pi"] - truth["cell_share"]).max()), absent_share=float(f["pi"][V - 1]),
         d=float(f["d"]), d_true=truth["doublet_rate"], het_rate=float(f["d"] * (1 - np.sum(f["pi"] ** 2))), het_rate_true=truth["heterotypic_rate"],
         right_best=right["BEST"] / n, right_call=right["CALL"] / n, singlets_called_doublets_best=sng_as_dbl["BEST"] / max(n_sng, 1),
         singlets_called_doublets_call=sng_as_dbl["CALL"] / max(n_sng, 1), het_recall_best=het_found["BEST"] / max(n_het, 1),
         het_recall_call=het_found["CALL"] / max(n_het, 1), min_post=0.9, wall_s=round(wall, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "prior_bench.jsonl"))
    a = ap.parse_args()
    import torch
    from demuxlet_amd import build, engine, prior, synth
    build.build()
    dev = torch.device("cuda", 0)

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    for name, sz in SIZES.items():
        B, V, A = sz["B"], sz["V"], sz["A"]
        grid = device_grid(torch, dev, B, V, A, 0xEB + V)
        nbytes = grid.numel() * 8
        dst = torch.empty_like(grid)
        torch.cuda.synchronize()
        e = engine.Engine(V, (0.0, 0.5))
        ptr = int(grid.data_ptr())
        pi, d = np.full(V, 1.0 / V), 0.1
        es, fo, cp = [], [], []
        for i in range(a.warmup + a.reps):
            e.prior_step(pi, d, grid=ptr, n_cells=B)
            inf = e.prior_info()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(); dst.copy_(grid); ev1.record(); torch.cuda.synchronize()
            if i >= a.warmup:
                es.append(inf["estep_ms"]); fo.append(inf["fold_ms"]); cp.append(ev0.elapsed_time(ev1))
        e_ms, f_ms, c_ms = statistics.median(es), statistics.median(fo), statistics.median(cp)
        calls = []
        for i in range(a.warmup + a.reps):
            e.prior_call(pi, d, grid=ptr, n_cells=B)
            if i >= a.warmup:
                calls.append(e.prior_info()["call_ms"])
        emit(what="iteration", size=name, B=B, V=V, A=A, grid_bytes=nbytes, reps=len(es), estep_ms=round(e_ms, 4), estep_ms_min=round(min(es), 4),
             estep_ms_max=round(max(es), 4), fold_ms=round(f_ms, 4), iter_ms=round(e_ms + f_ms, 4), estep_gb_s=round(nbytes / e_ms / 1e6, 1),
             iter_gb_s=round(nbytes / (e_ms + f_ms) / 1e6, 1), d2d_copy_ms=round(c_ms, 4), d2d_copy_gb_s_read=round(nbytes / c_ms / 1e6, 1),
             d2d_copy_gb_s_moved=round(2 * nbytes / c_ms / 1e6, 1), call_ms=round(statistics.median(calls), 4),
             waves_per_block=e.prior_info()["waves_per_block"])
        t0 = time.perf_counter()
        f = e.prior_fit(grid=ptr, n_cells=B, d0=0.1, max_iter=200, tol=1e-6)
        wall = time.perf_counter() - t0
        inf = e.prior_info()
        emit(what="fit", size=name, B=B, V=V, A=A, n_iter=f["n_iter"], converged=bool(f["converged"]), d=float(f["d"]), fit_kernel_ms=round(inf["fit_ms"], 3),
             wall_ms=round(wall * 1e3, 3), ms_per_iter_wall=round(wall * 1e3 / (f["n_iter"] + 1), 4))
        e.close()
        del grid, dst
        torch.cuda.empty_cache()
    if not a.no_quality:
        for n in (30, 300):
            quality(engine, prior, synth, a.out, n, emit)


if __name__ == "__main__":
    main()
