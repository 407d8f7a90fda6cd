"""Per-barcode ambient RNA contamination ("soup") from the allele data the engine already holds.

Soup is the average of many lysed cells, so at SNP i its reads show ALT with a fixed frequency a_i.  A droplet called as sample v with
a fraction rho of soup reads has, at SNP i, ALT probability p_g(rho) = (1 - rho) g / 2 + rho a_i under each genotype g of v.  The engine
computes the log-likelihood of every assigned barcode's reads over a grid of rho (Engine.ambient_profile, dmx_engine_ambient; DESIGN.md
section 14); this module builds a, reads the profile into per-barcode estimates and a pool estimate, and writes them:

  <prefix>.ambient.tsv       BARCODE SM_ID N.SNP N.READ RHO RHO.LO RHO.HI LLK.RHO LLK.0 LLR — one row per assigned barcode
  <prefix>.ambient_pool.tsv  RHO LLK per grid point: the sum of the assigned barcodes' profiles, then the pool estimate

RHO is the grid point of the highest LL (the lowest one on ties), RHO.LO / RHO.HI the smallest and largest grid points whose LL is within
1.92 (half the 95 % chi-square quantile of one degree of freedom) of that maximum, LLK.0 the LL at rho = 0 and LLR = LLK.RHO - LLK.0.
A doublet called as a singlet also looks like a high-rho singlet: a high RHO is a QC signal, not a proof of soup.

    python -m demuxlet_amd.ambient --pileup <x>.pileup.txt --out <prefix> [--best <x>.best] [--min-prb P] [--ambient reads|genotypes]
        [--grid-max 0.5] [--grid-step 0.01 | --grid R ...] [--alpha A ...] [--fast] [--gpu G]

reads the dump that `demuxlet --pileup-only` writes.  Without --best, the unchanged demultiplexing pass runs first and writes
<prefix>.best/.single/.sing2; its singlets are the barcodes profiled."""
from __future__ import annotations

import argparse
import sys
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import capi, engine, refine

MAX_GRID = 256              # dmx_engine_ambient's longest grid
CI_DROP = 1.92              # RHO.LO / RHO.HI: grid points with LL >= max - CI_DROP
AMBIENT_HEADER = "BARCODE\tSM_ID\tN.SNP\tN.READ\tRHO\tRHO.LO\tRHO.HI\tLLK.RHO\tLLK.0\tLLR\n"
POOL_HEADER = "RHO\tLLK\n"


def default_grid(grid_max: float = 0.5, grid_step: float = 0.01) -> np.ndarray:
    """0, step, 2 step, ... up to grid_max (51 points by default)."""
    if not (grid_step > 0.0) or not (0.0 <= grid_max <= 1.0):
        raise ValueError(f"grid: step {grid_step} must be > 0 and max {grid_max} in [0, 1]")
    n = int(np.floor(grid_max / grid_step + 1e-9)) + 1
    return check_grid(np.round(np.arange(n) * grid_step, 12))


def check_grid(grid) -> np.ndarray:
    g = np.ascontiguousarray(grid, dtype=np.float64)
    if g.ndim != 1 or not 1 <= len(g) <= MAX_GRID:
        raise ValueError(f"grid: 1 to {MAX_GRID} points, got {g.size}")
    if not np.all((g >= 0.0) & (g <= 1.0)):
        raise ValueError("grid: every point must be in [0, 1]")
    if len(g) > 1 and not np.all(np.diff(g) > 0.0):
        raise ValueError("grid: points must be strictly ascending")
    return g


def check_ambient(a, n_snps: int) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (n_snps,):
        raise ValueError(f"ambient: {a.shape} for {n_snps} SNPs")
    if not np.all((a >= 0.0) & (a <= 1.0)):
        raise ValueError("ambient: every frequency must be in [0, 1]")
    return a


def check_assign(assign, n_cells: int, n_samples: int) -> np.ndarray:
    a = np.ascontiguousarray(assign, dtype=np.int32)
    if a.shape != (n_cells,):
        raise ValueError(f"assign: {a.shape} for {n_cells} barcodes")
    if a.size and (a.min() < -1 or a.max() >= n_samples):
        raise ValueError(f"assign: sample indices must be in [-1, {n_samples})")
    return a


def ambient_from_counts(n_ref, n_alt) -> np.ndarray:
    """a_i = (n_alt + 1) / (n_ref + n_alt + 2): the pooled ALT fraction of every barcode's stored reads."""
    r = np.asarray(n_ref, dtype=np.float64)
    x = np.asarray(n_alt, dtype=np.float64)
    return (x + 1.0) / (r + x + 2.0)


def ambient_from_genotypes(g, assign) -> np.ndarray:
    """a_i = sum over v of pi_v (gp[i][v][1] / 2 + gp[i][v][2]), pi_v the fraction of the assigned barcodes called v."""
    g = np.asarray(g, dtype=np.float64)
    a = np.asarray(assign)
    n = np.bincount(a[a >= 0], minlength=g.shape[1]).astype(np.float64)
    if n.sum() == 0:
        raise ValueError("ambient from genotypes: no assigned barcode")
    pi = n / n.sum()
    return np.clip((g[:, :, 1] * 0.5 + g[:, :, 2]) @ pi, 0.0, 1.0)


def ambient_from_reads(eng: engine.Engine, g: np.ndarray) -> np.ndarray:
    """ambient_from_counts over the engine's staged pileup: one refinement with every barcode in column 0 (as cluster.py's prior)."""
    _, _, n_ref, n_alt, _ = eng.refine_genotypes(np.zeros(eng.B, dtype=np.int32), g)
    return ambient_from_counts(n_ref[:, 0], n_alt[:, 0])


@dataclass
class Summary:
    """Per-barcode estimates from a profile ll[B][Q] (rows of unassigned barcodes are meaningless)."""
    rho: np.ndarray          # grid point of the highest LL, lowest on ties
    rho_lo: np.ndarray       # smallest grid point with LL >= max - CI_DROP
    rho_hi: np.ndarray       # largest one
    llk_rho: np.ndarray
    llk_0: np.ndarray        # LL at rho = 0 (NaN when the grid has no 0)
    llr: np.ndarray


def summarize(ll: np.ndarray, grid) -> Summary:
    ll = np.asarray(ll, dtype=np.float64)
    g = check_grid(grid)
    if ll.ndim != 2 or ll.shape[1] != len(g):
        raise ValueError(f"profile {ll.shape} for a grid of {len(g)}")
    B = ll.shape[0]
    top = np.argmax(ll, axis=1) if B else np.zeros(0, dtype=np.int64)
    mx = ll[np.arange(B), top]
    inside = ll >= (mx - CI_DROP)[:, None]
    lo = np.argmax(inside, axis=1) if B else top
    hi = len(g) - 1 - np.argmax(inside[:, ::-1], axis=1) if B else top
    l0 = ll[:, 0] if g[0] == 0.0 else np.full(B, np.nan)
    return Summary(g[top], g[lo], g[hi], mx, l0, mx - l0)


def pool_profile(ll: np.ndarray, assign) -> np.ndarray:
    """sum over the assigned barcodes of ll[b], added serially in ascending cell id."""
    ll = np.asarray(ll, dtype=np.float64)
    sel = ll[np.asarray(assign) >= 0]
    if len(sel) == 0:
        return np.zeros(ll.shape[1])
    return np.cumsum(sel, axis=0)[-1]


def write_ambient_tsv(path: str, barcodes: Sequence[str], sample_ids: Sequence[str], assign, n_snp, n_read, s: Summary) -> None:
    """One row per assigned barcode, in cell id order."""
    with open(path, "w") as f:
        f.write(AMBIENT_HEADER)
        for b in np.flatnonzero(np.asarray(assign) >= 0):
            f.write(f"{barcodes[b]}\t{sample_ids[int(assign[b])]}\t{int(n_snp[b])}\t{int(n_read[b])}\t{s.rho[b]:.4f}\t{s.rho_lo[b]:.4f}\t"
                    f"{s.rho_hi[b]:.4f}\t{s.llk_rho[b]:.5f}\t{s.llk_0[b]:.5f}\t{s.llr[b]:.5f}\n")


def write_pool_tsv(path: str, grid, pool: np.ndarray) -> float:
    """RHO LLK per grid point, then a `#RHO.POOL` line with the argmax (lowest on ties); returns it."""
    g = check_grid(grid)
    est = float(g[int(np.argmax(pool))])
    with open(path, "w") as f:
        f.write(POOL_HEADER)
        for r, x in zip(g, pool):
            f.write(f"{r:.4f}\t{x:.5f}\n")
        f.write(f"#RHO.POOL\t{est:.4f}\n")
    return est


def ambient_run(store_or_pileup, g: np.ndarray, sample_ids: Sequence[str], out_prefix: str, best: Optional[str] = None, ambient="reads",
                grid=None, min_prb: float = 0.0, alphas: Sequence[float] = (0.0, 0.5), barcodes: Optional[Sequence[str]] = None,
                device: int = 0, mode: int = capi.DMX_MODE_STRICT, **demuxlet_run_kwargs):
    """Profile the singlets of `best` (a `.best` path) against genotype matrix g.  Without `best`, the unchanged demuxlet_run writes
    <out_prefix>.best/.single/.sing2 first and its `.best` is used.  `ambient` is "reads", "genotypes" or an array of n_snps frequencies.
    `store_or_pileup` is a Store, or a HostPileup with barcodes=... as for demuxlet_run.  Writes <out_prefix>.ambient.tsv and
    .ambient_pool.tsv; returns a dict with the profile, counts, summary, pool profile and pool estimate."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    grid = default_grid() if grid is None else check_grid(grid)
    if isinstance(ambient, str) and ambient not in ("reads", "genotypes"):
        raise ValueError(f"ambient: 'reads', 'genotypes' or an array, not {ambient!r}")
    if isinstance(store_or_pileup, engine.HostPileup):
        pl = store_or_pileup
        if barcodes is None:
            raise ValueError("ambient_run: a HostPileup needs barcodes=")
    else:
        pl, barcodes = store_or_pileup.freeze(), store_or_pileup.barcodes()
    if g.ndim != 3 or g.shape[0] != pl.n_snps or g.shape[1] != len(sample_ids) or g.shape[2] != 3:
        raise ValueError(f"genotype matrix {g.shape} for {pl.n_snps} SNPs and {len(sample_ids)} samples")
    if not isinstance(ambient, str):
        ambient = check_ambient(ambient, pl.n_snps)
    if best is None:
        engine.demuxlet_run(pl, g, sample_ids, alphas, out_prefix, barcodes=barcodes, device=device, mode=mode, **demuxlet_run_kwargs)
        best = out_prefix + ".best"
    assign = refine.assignments_from_best(best, sample_ids, barcodes, min_prb)
    eng = engine.Engine(len(sample_ids), alphas, device=device, mode=mode)
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        if isinstance(ambient, str):
            a = ambient_from_reads(eng, g) if ambient == "reads" else ambient_from_genotypes(g, assign)
        else:
            a = ambient
        ll, n_snp, n_read = eng.ambient_profile(assign, a, grid)
    finally:
        eng.close()
    s = summarize(ll, grid)
    pool = pool_profile(ll, assign)
    write_ambient_tsv(out_prefix + ".ambient.tsv", barcodes, sample_ids, assign, n_snp, n_read, s)
    est = write_pool_tsv(out_prefix + ".ambient_pool.tsv", grid, pool)
    return dict(assign=assign, ambient=a, grid=grid, ll=ll, n_snp=n_snp, n_read=n_read, summary=s, pool=pool, pool_rho=est)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.ambient", description="per-barcode ambient RNA contamination from allele data")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.ambient.tsv, <out>.ambient_pool.tsv (and <out>.best/... without --best)")
    ap.add_argument("--best", help="a .best of this pileup: its singlets are profiled (default: run the demultiplexing pass first)")
    ap.add_argument("--min-prb", type=float, default=0.0, help="use only singlets with PRB.SNG1 >= this (default: all SNG- calls)")
    ap.add_argument("--ambient", choices=("reads", "genotypes"), default="reads",
                    help="soup ALT frequency: pooled reads of every barcode (default) or the singlet-weighted genotype mean")
    ap.add_argument("--grid-max", type=float, default=0.5, help="largest contamination fraction of the default grid (default 0.5)")
    ap.add_argument("--grid-step", type=float, default=0.01, help="step of the default grid (default 0.01)")
    ap.add_argument("--grid", type=float, nargs="+", help="explicit grid of contamination fractions (replaces --grid-max / --grid-step)")
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.0, 0.5], help="doublet grid of the demultiplexing pass (default 0 0.5)")
    ap.add_argument("--fast", action="store_true", help="DMX_MODE_FAST for the demultiplexing pass")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    if not 0.0 <= a.min_prb <= 1.0:
        ap.error("--min-prb must be in [0, 1]")
    try:
        a.grid = check_grid(a.grid) if a.grid is not None else default_grid(a.grid_max, a.grid_step)
    except ValueError as ex:
        ap.error(str(ex))
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    d = refine.read_pileup_txt(a.pileup)
    r = ambient_run(d.pileup, d.g, d.sample_ids, a.out, best=a.best, ambient=a.ambient, grid=a.grid, min_prb=a.min_prb, alphas=a.alpha,
                    barcodes=d.barcodes, device=a.gpu, mode=capi.DMX_MODE_FAST if a.fast else capi.DMX_MODE_STRICT)
    print(f"{int((r['assign'] >= 0).sum())} barcodes profiled; pool rho = {r['pool_rho']:.4f}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
