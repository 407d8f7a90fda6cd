"""Donor shares of a read pool: which donors, in what proportions, make up a group of barcodes' reads.

Every stored read of a group is taken as an independent draw from a mixture of the V donors (the model ambient.py uses for soup): at SNP i
a read is ALT with probability A_i(w) = sum over v of w_v d_iv, d_iv the expected ALT dosage of donor v from the genotype matrix.  The
engine finds the maximum-likelihood shares by an EM whose iteration is one pass over the pileup (Engine.census, dmx_engine_census;
DESIGN.md section 22), accelerated by SQUAREM and stopped by the duality gap, an upper bound of the log-likelihood still to be gained.
Uses: the make-up of the soup (a group of empty droplets), the donors' cell or RNA contributions (all barcodes pooled), and whether a
donor of the VCF is in the pool at all (a share of 0).

    python -m demuxlet_amd.census --pileup <x>.pileup.txt --out <prefix> [--groups FILE | --max-reads N] [--tol T] [--max-steps M]
        [--no-accel] [--gpu G]

reads the dump that `demuxlet --pileup-only` writes.  By default every barcode goes into one group POOL; --groups names a
BARCODE<TAB>GROUP file (barcodes not listed are left out); --max-reads N makes two groups, EMPTY (barcodes with at most N unique reads)
and CELLS.  It writes

  <prefix>.census.tsv          GROUP SM_ID SHARE READS — one row per group and donor; READS = SHARE x the group's counted reads
  <prefix>.census_groups.tsv   GROUP N.BARCODE N.SNP N.READ LLK GAP STEPS CONVERGED — N.SNP counts the (barcode, SNP) pairs that contributed
  <prefix>.census_profile.tsv  SNP GROUP A — the implied ALT frequency sum_v w_v d_iv of every SNP (NA where a donor's genotype row is
                               all zero: such SNPs are left out of the census)"""
from __future__ import annotations

import argparse
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import engine, refine

CENSUS_HEADER = "GROUP\tSM_ID\tSHARE\tREADS\n"
GROUPS_HEADER = "GROUP\tN.BARCODE\tN.SNP\tN.READ\tLLK\tGAP\tSTEPS\tCONVERGED\n"
PROFILE_HEADER = "SNP\tGROUP\tA\n"
MAX_GROUPS = 1024           # dmx_engine_census's most groups


def dosage(g) -> Tuple[np.ndarray, np.ndarray]:
    """(d[S][V] float64, valid[S]) as the engine forms them: d = (gp1 / 2 + gp2) / ((gp0 + gp1) + gp2); a SNP where a donor's row does
    not sum to a positive finite number is invalid (its d entries are 0)."""
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    if g.ndim != 3 or g.shape[2] != 3:
        raise ValueError(f"genotype matrix {g.shape}: [S][V][3] expected")
    den = (g[:, :, 0] + g[:, :, 1]) + g[:, :, 2]
    ok = (den > 0.0) & np.isfinite(den)
    with np.errstate(all="ignore"):
        d = np.where(ok, (g[:, :, 1] * 0.5 + g[:, :, 2]) / np.where(ok, den, 1.0), 0.0)
    return d, ok.all(axis=1)


def ambient_profile(w, g) -> np.ndarray:
    """The ALT frequency a pool of shares w[V] implies at every SNP: A_i = sum over v of w_v d_iv (NaN at an invalid SNP)."""
    w = np.asarray(w, dtype=np.float64)
    d, valid = dosage(g)
    if w.shape != (d.shape[1],):
        raise ValueError(f"shares {w.shape} for {d.shape[1]} samples")
    A = np.zeros(d.shape[0])
    for v in range(d.shape[1]):                     # (the engine's order: ascending v, every product and sum rounded)
        A = A + w[v] * d[:, v]
    return np.where(valid, A, np.nan)


def read_groups(path: str, barcodes: Sequence[str]) -> Tuple[np.ndarray, List[str]]:
    """A BARCODE<TAB>GROUP file -> (group[B] int32, -1 for barcodes not listed; group names in order of first appearance).  Empty lines
    and lines starting with # are skipped; an unknown barcode, a barcode listed twice or a malformed line is an error."""
    cmap = {b: c for c, b in enumerate(barcodes)}
    group = np.full(len(barcodes), -1, dtype=np.int32)
    names: List[str] = []
    idx = {}
    with open(path) as f:
        for n, line in enumerate(f, 1):
            line = line.rstrip("\n")
            if not line or line.startswith("#"):
                continue
            t = line.split("\t")
            if len(t) != 2 or not t[0] or not t[1]:
                raise ValueError(f"{path}:{n}: BARCODE<TAB>GROUP expected")
            c = cmap.get(t[0])
            if c is None:
                raise ValueError(f"{path}:{n}: barcode {t[0]!r} not in this pileup")
            if group[c] >= 0:
                raise ValueError(f"{path}:{n}: barcode {t[0]!r} listed twice")
            if t[1] not in idx:
                idx[t[1]] = len(names)
                names.append(t[1])
            group[c] = idx[t[1]]
    if not names:
        raise ValueError(f"{path}: no group")
    if len(names) > MAX_GROUPS:
        raise ValueError(f"{path}: {len(names)} groups, at most {MAX_GROUPS}")
    return group, names


def split_by_reads(rd_uniq, max_reads: int) -> Tuple[np.ndarray, List[str]]:
    """Two groups: EMPTY (0) = barcodes with at most max_reads unique reads, CELLS (1) = the others."""
    if max_reads < 0:
        raise ValueError("max_reads must be >= 0")
    return (np.asarray(rd_uniq) > max_reads).astype(np.int32), ["EMPTY", "CELLS"]


def write_census_tsv(path: str, names: Sequence[str], sample_ids: Sequence[str], w: np.ndarray, n_read) -> None:
    with open(path, "w") as f:
        f.write(CENSUS_HEADER)
        for k, name in enumerate(names):
            for v, s in enumerate(sample_ids):
                f.write(f"{name}\t{s}\t{w[k, v]:.6f}\t{w[k, v] * float(n_read[k]):.2f}\n")


def write_groups_tsv(path: str, names: Sequence[str], n_bar, r: dict) -> None:
    with open(path, "w") as f:
        f.write(GROUPS_HEADER)
        for k, name in enumerate(names):
            f.write(f"{name}\t{int(n_bar[k])}\t{int(r['n_pair'][k])}\t{int(r['n_read'][k])}\t{r['ll'][k]:.5f}\t{r['gap'][k]:.3g}\t"
                    f"{int(r['n_steps'][k])}\t{int(r['converged'][k])}\n")


def write_profile_tsv(path: str, names: Sequence[str], profile: np.ndarray, snps=None) -> None:
    """profile[G][S]; the SNP column is `rid:pos` when the dump's SNP records are given, the SNP id otherwise."""
    with open(path, "w") as f:
        f.write(PROFILE_HEADER)
        for i in range(profile.shape[1]):
            sid = f"{snps[i][0]}:{snps[i][1]}" if snps is not None else str(i)
            for k, name in enumerate(names):
                a = profile[k, i]
                f.write(f"{sid}\t{name}\t{'NA' if np.isnan(a) else format(a, '.6f')}\n")


def census_run(store_or_pileup, g: np.ndarray, sample_ids: Sequence[str], out_prefix: Optional[str], groups=None, max_reads: Optional[int] = None,
               tol: float = 1e-4, max_steps: int = 2000, accelerate: bool = True, gpu: int = 0, barcodes: Optional[Sequence[str]] = None,
               snps=None) -> dict:
    """The census of `store_or_pileup` (a Store, or a HostPileup) against genotype matrix g.  `groups` is None (one group POOL of every
    barcode), a BARCODE<TAB>GROUP path (needs the barcodes: a Store's own, or barcodes=), or a pair (group[B] int array, names);
    max_reads=N instead makes the groups EMPTY / CELLS.  Writes the three files unless out_prefix is None; returns a dict with the
    engine's results (w, ll, gap, n_steps, converged, n_read, n_pair), group, names, n_barcode, profile[G][S] and info."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    if groups is not None and max_reads is not None:
        raise ValueError("census_run: groups and max_reads exclude each other")
    if isinstance(store_or_pileup, engine.HostPileup):
        pl = store_or_pileup
    else:
        pl, barcodes = store_or_pileup.freeze(), store_or_pileup.barcodes()
    if g.ndim != 3 or g.shape[0] != pl.n_snps or g.shape[1] != len(sample_ids) or g.shape[2] != 3:
        raise ValueError(f"genotype matrix {g.shape} for {pl.n_snps} SNPs and {len(sample_ids)} samples")
    if max_reads is not None:
        group, names = split_by_reads(pl.rd_uniq, max_reads)
    elif groups is None:
        group, names = np.zeros(pl.n_cells, dtype=np.int32), ["POOL"]
    elif isinstance(groups, str):
        if barcodes is None:
            raise ValueError("census_run: a groups file with a HostPileup needs barcodes=")
        group, names = read_groups(groups, barcodes)
    else:
        group, names = np.ascontiguousarray(groups[0], dtype=np.int32), list(groups[1])
        if group.shape != (pl.n_cells,) or (group.size and (group.min() < -1 or group.max() >= len(names))):
            raise ValueError(f"groups: {pl.n_cells} entries in [-1, {len(names)}) expected")
    if not 1 <= len(names) <= MAX_GROUPS:
        raise ValueError(f"census_run: {len(names)} groups, 1 to {MAX_GROUPS} expected")
    eng = engine.Engine(len(sample_ids), device=gpu)
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        r = eng.census(group, n_groups=len(names), tol=tol, max_steps=max_steps, accelerate=accelerate)
        info = eng.census_info()
    finally:
        eng.close()
    profile = np.stack([ambient_profile(r["w"][k], g) for k in range(len(names))])
    n_bar = np.bincount(group[group >= 0], minlength=len(names))
    if out_prefix is not None:
        write_census_tsv(out_prefix + ".census.tsv", names, sample_ids, r["w"], r["n_read"])
        write_groups_tsv(out_prefix + ".census_groups.tsv", names, n_bar, r)
        write_profile_tsv(out_prefix + ".census_profile.tsv", names, profile, snps)
    return dict(r, group=group, names=names, n_barcode=n_bar, profile=profile, info=info)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.census", description="donor shares of a pool of reads")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.census.tsv, <out>.census_groups.tsv, <out>.census_profile.tsv")
    ap.add_argument("--groups", help="BARCODE<TAB>GROUP file (default: one group POOL of every barcode)")
    ap.add_argument("--max-reads", type=int, help="two groups: EMPTY = barcodes with at most N unique reads, CELLS = the others")
    ap.add_argument("--tol", type=float, default=1e-4, help="stop a group at duality gap <= this, in log-likelihood units (default 1e-4)")
    ap.add_argument("--max-steps", type=int, default=2000, help="passes per group at most (default 2000)")
    ap.add_argument("--no-accel", action="store_true", help="plain EM instead of SQUAREM")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    if a.groups is not None and a.max_reads is not None:
        ap.error("--groups and --max-reads exclude each other")
    if a.max_reads is not None and a.max_reads < 0:
        ap.error("--max-reads must be >= 0")
    if not a.tol > 0.0:
        ap.error("--tol must be > 0")
    if a.max_steps < 1:
        ap.error("--max-steps must be >= 1")
    if a.gpu < 0:
        ap.error("--gpu must be >= 0")
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    d = refine.read_pileup_txt(a.pileup)
    r = census_run(d.pileup, d.g, d.sample_ids, a.out, groups=a.groups, max_reads=a.max_reads, tol=a.tol, max_steps=a.max_steps,
                   accelerate=not a.no_accel, gpu=a.gpu, barcodes=d.barcodes, snps=d.snps)
    for k, name in enumerate(r["names"]):
        top = int(np.argmax(r["w"][k]))
        print(f"{name}: {int(r['n_read'][k])} reads, {int(r['n_steps'][k])} steps, gap {r['gap'][k]:.3g}; largest share "
              f"{d.sample_ids[top]} {r['w'][k, top]:.4f}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
