"""Site audit: per-SNP goodness of fit, and a re-run without the sites that misfit.

Every pass takes the genotype matrix's rows as given.  fit.py asks whether a barcode's call explains that barcode's reads, summed over
its SNPs; this module asks the transposed question: does this SNP's row explain the reads the pool holds there, summed over the barcodes?
Rows that are wrong at the site level — REF and ALT exchanged or on the wrong strand, a paralogous or RNA-edited site with ALT reads
nobody's genotype predicts, strong reference bias — are the commonest way a genotype-based run degrades.  The engine
(Engine.site_fit, dmx_engine_site_fit) gives, per SNP, fit.py's three sums over the barcodes that cover it under
their own calls, and the signed excess of ALT reads over their expectation with its variance:

  Z = (LLK.OBS - LLK.EXP) / LLK.SD,   P = erfc(-Z / sqrt 2) / 2,   Z.ALT = ALT.EXC / ALT.SD  (> 0: unexplained ALT reads, < 0: missing ones),
  FLAG = MISFIT when N.CELL >= --min-cells and Z < --z-min.

Each barcode's hypothesis is fit.py's (its BEST call; --singlets-only leaves the doublet hypotheses out).

  <prefix>.sites.tsv         RID POS REF ALT N.CELL N.READ N.ALT N.TRUNC N.ZERO LLK.OBS LLK.EXP LLK.SD Z P ALT.EXC ALT.SD Z.ALT FLAG — one row
                             per SNP, in SNP order; NA where a variance is 0; the last round's audit
  <prefix>.sites_rounds.tsv  ROUND N.FLAG N.RELEASED N.NEW N.BEST.CHANGED — one row per round
  <prefix>.r<r>.best/...     round r's calls, by the unchanged demultiplexing pass on the pileup without the flagged SNPs' pairs

--rounds R iterates: round 0 is the unchanged demultiplexing pass (or --best); round r audits ALL SNPs under round r - 1's calls (a
site flagged on the strength of wrong calls can be released again), drops the flagged SNPs' pairs from the pileup on the host and calls
again.  Z is conservative (above 0, compressed) where the true genotypes are known better than the matrix says, and at about 30 cells
per SNP its lower tail is heavier than normal (one or two base-call errors reach -4): --z-min and --min-cells are knobs, not p-values.
Limits: Z is pooled over the donors at a site; a swap is invisible where every covering donor is heterozygous; no per-(SNP, donor)
rows (refine.py's job); one GPU.

    python -m demuxlet_amd.sites --pileup <x>.pileup.txt --out <prefix> [--best <x>.best] [--rounds 1] [--max-reads 4] [--z-min -6]
        [--min-cells 10] [--singlets-only] [--ambient-tsv <x>.ambient.tsv [--ambient reads|genotypes|census]] [--alpha A ...] [--fast] [--gpu G]"""
from __future__ import annotations

import argparse
import math
import sys
from typing import Optional, Sequence

import numpy as np

from . import capi, engine, fit, refine

MAX_READS = fit.MAX_READS
SITES_HEADER = "RID\tPOS\tREF\tALT\tN.CELL\tN.READ\tN.ALT\tN.TRUNC\tN.ZERO\tLLK.OBS\tLLK.EXP\tLLK.SD\tZ\tP\tALT.EXC\tALT.SD\tZ.ALT\tFLAG\n"
ROUNDS_HEADER = "ROUND\tN.FLAG\tN.RELEASED\tN.NEW\tN.BEST.CHANGED\n"


def drop_snps(pileup: engine.HostPileup, mask) -> engine.HostPileup:
    """The pileup without the pairs at the SNPs of mask[n_snps] (True = drop), in the sparse layout (also for a dense input and an empty
    mask); n_snps and the rd_* counters are unchanged."""
    mask = np.asarray(mask, dtype=bool)
    if mask.shape != (pileup.n_snps,):
        raise ValueError(f"mask: {mask.shape} for {pileup.n_snps} SNPs")
    po = np.asarray(pileup.cell_pair_off, dtype=np.int64)
    nrd = np.asarray(pileup.pair_nrd)
    cell = np.repeat(np.arange(pileup.n_cells), np.diff(po))
    snp = np.asarray(pileup.pair_snp, dtype=np.int32) if pileup.pair_snp is not None else (np.arange(len(cell)) - po[cell]).astype(np.int32)
    keep = ~mask[snp]
    n64 = nrd.astype(np.int64)
    new_po = np.concatenate([[0], np.cumsum(np.bincount(cell[keep], minlength=pileup.n_cells))]).astype(np.int64)
    new_ro = np.concatenate([[0], np.cumsum(np.bincount(cell[keep], weights=n64[keep], minlength=pileup.n_cells))]).astype(np.int64)
    reads = np.asarray(pileup.reads, dtype=np.uint8)[np.repeat(keep, n64)]
    return engine.HostPileup(pileup.n_cells, pileup.n_snps, new_po, new_ro, np.ascontiguousarray(snp[keep]), np.ascontiguousarray(nrd[keep]),
                             np.ascontiguousarray(reads), pileup.rd_totl, pileup.rd_pass, pileup.rd_uniq)


def site_scores(r: dict, z_min: float, min_cells: int):
    """(Z, P, Z.ALT, flag) per SNP from Engine.site_fit's dict."""
    z = fit.z_scores(r["obs"], r["mean"], r["var"])
    za = fit.z_scores(r["exc"], np.zeros_like(r["exc"]), r["vexc"])
    with np.errstate(invalid="ignore"):
        flag = (np.asarray(r["n_cell"]) >= min_cells) & (z < z_min)
    return z, fit.lower_tail(z), za, flag


def _sd(v) -> float:
    return math.sqrt(v) if np.isfinite(v) and v > 0.0 else 0.0


def write_sites_tsv(path: str, snps: Sequence, r: dict, z, p, z_alt, flag) -> int:
    """One row per SNP, in SNP order; returns the number of MISFIT rows."""
    num = fit._num
    with open(path, "w") as f:
        f.write(SITES_HEADER)
        for i, (rid, pos, ref, alt) in enumerate(snps):
            f.write(f"{rid}\t{pos}\t{ref}\t{alt}\t{int(r['n_cell'][i])}\t{int(r['n_read'][i])}\t{int(r['n_alt'][i])}\t{int(r['n_trunc'][i])}\t"
                    f"{int(r['n_zero'][i])}\t{num(r['obs'][i], '.5f')}\t{num(r['mean'][i], '.5f')}\t{_sd(r['var'][i]):.5f}\t{num(z[i], '.4f')}\t"
                    f"{num(p[i], '.4g')}\t{num(r['exc'][i], '.5f')}\t{_sd(r['vexc'][i]):.5f}\t{num(z_alt[i], '.4f')}\t{'MISFIT' if flag[i] else '.'}\n")
    return int(np.sum(flag))


def write_rounds_tsv(path: str, rounds: Sequence[dict]) -> None:
    with open(path, "w") as f:
        f.write(ROUNDS_HEADER)
        for k in rounds:
            f.write(f"{k['round']}\t{k['n_flag']}\t{k['n_released']}\t{k['n_new']}\t{k['n_best_changed']}\n")


def hypotheses(rows: fit.BestHyp, singlets_only: bool):
    """(hyp, alpha) of a `.best`'s rows; with singlets_only the doublet hypotheses become unused barcodes."""
    hyp, alpha = rows.hyp.copy(), rows.alpha.copy()
    if singlets_only:
        d = hyp[:, 1] >= 0
        hyp[d] = (-1, -1)
        alpha[d] = 0.0
    return hyp, alpha


def site_run(store_or_pileup, g: np.ndarray, sample_ids: Sequence[str], out_prefix: str, snps: Optional[Sequence] = None,
             best: Optional[str] = None, rounds: int = 1, max_reads: int = 4, z_min: float = -6.0, min_cells: int = 10,
             singlets_only: bool = False, rho=None, ambient="reads", alphas: Sequence[float] = (0.0, 0.5),
             barcodes: Optional[Sequence[str]] = None, device: int = 0, mode: int = capi.DMX_MODE_STRICT, partial_bytes: int = 0,
             **demuxlet_run_kwargs):
    """Audit every SNP's row of g under the calls of `best` (a `.best` path; without it the unchanged demuxlet_run writes
    <out_prefix>.best/.single/.sing2 first: round 0).  Round r = 1..rounds audits all SNPs of the full pileup under round r - 1's calls,
    flags, and lets the unchanged demuxlet_run call the pileup without the flagged SNPs' pairs into <out_prefix>.r<r>.best/.single/.sing2.
    `snps` is (rid, pos, ref, alt) per SNP for the table (default: (0, SNP id, ".", ".")); `rho` / `ambient` as for fit.fit_run.  Writes
    <out_prefix>.sites.tsv (the last round's audit) and .sites_rounds.tsv; returns a dict with every round's engine result, Z, flags and
    `.best` path."""
    from . import ambient as amb_mod
    g = np.ascontiguousarray(g, dtype=np.float32)
    if not 1 <= int(max_reads) <= MAX_READS:
        raise ValueError(f"max_reads: 1 to {MAX_READS}, not {max_reads}")
    if int(rounds) < 1:
        raise ValueError(f"rounds: at least 1, not {rounds}")
    if not np.isfinite(z_min):
        raise ValueError("z_min must be finite")
    if int(min_cells) < 0:
        raise ValueError("min_cells must not be negative")
    if isinstance(ambient, str) and ambient not in ("reads", "genotypes", "census"):
        raise ValueError(f"ambient: 'reads', 'genotypes', 'census' or an array, not {ambient!r}")
    if isinstance(store_or_pileup, engine.HostPileup):
        pl = store_or_pileup
        if barcodes is None:
            raise ValueError("site_run: a HostPileup needs barcodes=")
    else:
        pl, barcodes = store_or_pileup.freeze(), store_or_pileup.barcodes()
    if g.ndim != 3 or g.shape[0] != pl.n_snps or g.shape[1] != len(sample_ids) or g.shape[2] != 3:
        raise ValueError(f"genotype matrix {g.shape} for {pl.n_snps} SNPs and {len(sample_ids)} samples")
    if snps is None:
        snps = [(0, i, ".", ".") for i in range(pl.n_snps)]
    if len(snps) != pl.n_snps:
        raise ValueError(f"snps: {len(snps)} rows for {pl.n_snps} SNPs")
    if rho is not None:
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        if rho.shape != (pl.n_cells,) or not np.all((rho >= 0.0) & (rho <= 1.0)):
            raise ValueError(f"rho: {pl.n_cells} values in [0, 1]")
        if not isinstance(ambient, str):
            ambient = amb_mod.check_ambient(ambient, pl.n_snps)
    if best is None:
        engine.demuxlet_run(pl, g, sample_ids, alphas, out_prefix, barcodes=barcodes, device=device, mode=mode, **demuxlet_run_kwargs)
        best = out_prefix + ".best"
    prev_flag = np.zeros(pl.n_snps, dtype=bool)
    prev_rows = fit.read_best_hypotheses(best, sample_ids, barcodes)
    out_rounds, table = [], []
    eng = engine.Engine(len(sample_ids), alphas, device=device, mode=mode)
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        a = None
        if rho is not None:
            a = amb_mod._ambient_builder(ambient, eng, g, lambda: refine.assignments_from_best(best, sample_ids, barcodes)) if isinstance(ambient, str) else ambient
        for r in range(1, int(rounds) + 1):
            hyp, alpha = hypotheses(prev_rows, singlets_only)
            res = eng.site_fit(hyp, alpha, rho, a, max_reads, partial_bytes)
            info = eng.site_fit_info()
            z, p, za, flag = site_scores(res, z_min, min_cells)
            prefix = f"{out_prefix}.r{r}"
            engine.demuxlet_run(drop_snps(pl, flag), g, sample_ids, alphas, prefix, barcodes=barcodes, device=device, mode=mode, **demuxlet_run_kwargs)
            rows = fit.read_best_hypotheses(prefix + ".best", sample_ids, barcodes)
            changed = int(sum(x != y for x, y in zip(rows.best, prev_rows.best)))
            table.append(dict(round=r, n_flag=int(flag.sum()), n_released=int((prev_flag & ~flag).sum()), n_new=int((flag & ~prev_flag).sum()),
                              n_best_changed=changed))
            out_rounds.append(dict(site=res, info=info, z=z, p=p, z_alt=za, flag=flag, best=prefix + ".best", rows=rows))
            prev_flag, prev_rows = flag, rows
    finally:
        eng.close()
    last = out_rounds[-1]
    n_flag = write_sites_tsv(out_prefix + ".sites.tsv", snps, last["site"], last["z"], last["p"], last["z_alt"], last["flag"])
    write_rounds_tsv(out_prefix + ".sites_rounds.tsv", table)
    return dict(rounds=out_rounds, table=table, best0=best, n_misfit=n_flag, ambient=a)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.sites", description="site audit: per-SNP goodness of fit and a re-run without the sites that misfit")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.sites.tsv, <out>.sites_rounds.tsv, <out>.r<r>.best/... (and <out>.best/... without --best)")
    ap.add_argument("--best", help="a .best of this pileup: its calls are round 0 (default: run the demultiplexing pass first)")
    ap.add_argument("--rounds", type=int, default=1, help="audit and re-call this many times (default 1)")
    ap.add_argument("--max-reads", type=int, default=4, help=f"reads of a (barcode, SNP) pair that enter, 1..{MAX_READS} (default 4)")
    ap.add_argument("--z-min", type=float, default=-6.0, help="FLAG is MISFIT below this Z (default -6)")
    ap.add_argument("--min-cells", type=int, default=10, help="... and only with at least this many counted barcodes at the SNP (default 10)")
    ap.add_argument("--singlets-only", action="store_true", help="leave the barcodes called as doublets out of the audit")
    ap.add_argument("--ambient-tsv", help="<x>.ambient.tsv of an ambient.py run: its RHO per barcode is the soup fraction of the hypothesis")
    ap.add_argument("--ambient", choices=("reads", "genotypes", "census"), default=None,
                    help="soup ALT frequency, as for ambient.py (default reads); needs --ambient-tsv")
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.0, 0.5], help="doublet grid of the demultiplexing pass (default 0 0.5)")
    ap.add_argument("--fast", action="store_true", help="DMX_MODE_FAST for the demultiplexing pass")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    if not 1 <= a.max_reads <= MAX_READS:
        ap.error(f"--max-reads must be in [1, {MAX_READS}]")
    if a.rounds < 1:
        ap.error("--rounds must be at least 1")
    if not np.isfinite(a.z_min):
        ap.error("--z-min must be finite")
    if a.min_cells < 0:
        ap.error("--min-cells must not be negative")
    if a.ambient is not None and a.ambient_tsv is None:
        ap.error("--ambient needs --ambient-tsv")
    if a.ambient is None:
        a.ambient = "reads"
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    d = refine.read_pileup_txt(a.pileup)
    rho = fit.read_rho_tsv(a.ambient_tsv, d.barcodes) if a.ambient_tsv else None
    r = site_run(d.pileup, d.g, d.sample_ids, a.out, snps=d.snps, best=a.best, rounds=a.rounds, max_reads=a.max_reads, z_min=a.z_min,
                 min_cells=a.min_cells, singlets_only=a.singlets_only, rho=rho, ambient=a.ambient, alphas=a.alpha, barcodes=d.barcodes,
                 device=a.gpu, mode=capi.DMX_MODE_FAST if a.fast else capi.DMX_MODE_STRICT)
    for k in r["table"]:
        print(f"round {k['round']}: {k['n_flag']} SNPs MISFIT ({k['n_released']} released, {k['n_new']} new); {k['n_best_changed']} barcodes changed BEST",
              file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
