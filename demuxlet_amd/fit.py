"""Goodness of fit of every call: flag droplets that no donor explains.

Every other pass ranks hypotheses against each other; a barcode of a donor who is missing from the VCF, whose VCF column belongs to
somebody else, or whose genotypes are on the wrong build still gets a confident SNG- line, because the nearest wrong donor beats the
other wrong donors.  This module asks the absolute question: under the barcode's own call, how likely are the reads it holds, compared
with what that likelihood would be if the call were true?  The engine (Engine.fit_profile, dmx_engine_fit) gives,
per barcode, the log-likelihood LLK.OBS of each covered SNP's first --max-reads reads and its mean LLK.EXP and standard deviation
LLK.SD under the hypothesis, given the depths and base qualities the barcode actually has:

  Z = (LLK.OBS - LLK.EXP) / LLK.SD,   P = erfc(-Z / sqrt 2) / 2 (the lower tail),   FLAG = MISFIT when Z < --z-min.

Each barcode's hypothesis is its BEST call: SNG-j is donor j, DBL-a-b-alpha the pair at that share, AMB- the better of the two by the
`.best` file's own LLKs (LLK12 against SNG.LLK1).  A barcode not called SNG- is also scored as a singlet of SNG.1ST (Z.SNG1): a doublet
call that repairs a misfit shows as Z.SNG1 << Z.

  <prefix>.fit.tsv         BARCODE BEST HYP N.SNP N.READ N.TRUNC N.ZERO LLK.OBS LLK.EXP LLK.SD Z P Z.SNG1 FLAG — one row per barcode of the
                           `.best`, in byte-wise barcode order; NA where LLK.SD is 0
  <prefix>.fit_donors.tsv  SM_ID N.CELL MED.Z MIN.Z N.MISFIT FRAC.MISFIT — one row per sample over the barcodes hypothesised as its singlets,
                           one row DBL over the doublet hypotheses, then `#POOL` with the totals

A swapped column shows as one donor all of whose cells misfit; a missing donor as misfitting cells spread over the remaining donors, and
their number over the mean N.CELL is the figure to try after partial.py's --n-unknown.  Z sits above 0 for correct calls when the true
genotypes are known better than the matrix says (hard genotypes, a softened matrix): the test is conservative then.  Limits: one
hypothesis per barcode; reads beyond the first --max-reads of a pair are ignored (N.TRUNC counts the pairs); the hypothesis was chosen
because it fits best, which is not corrected for; homotypic doublets fit perfectly; no triplet hypotheses; one GPU.

    python -m demuxlet_amd.fit --pileup <x>.pileup.txt --out <prefix> [--best <x>.best] [--max-reads 4] [--z-min -4]
        [--ambient-tsv <x>.ambient.tsv [--ambient reads|genotypes|census]] [--alpha A ...] [--fast] [--gpu G]

reads the dump that `demuxlet --pileup-only` writes.  Without --best, the unchanged demultiplexing pass runs first and writes
<prefix>.best/.single/.sing2.  --ambient-tsv takes RHO per barcode from an earlier ambient.py run (0 for barcodes it does not list) and
scores every hypothesis with that fraction of soup; the soup's ALT frequencies come from ambient.py's builders."""
from __future__ import annotations

import argparse
import math
import sys
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import capi, engine, refine

MAX_READS = 8               # dmx_engine_fit's largest max_reads
FIT_HEADER = "BARCODE\tBEST\tHYP\tN.SNP\tN.READ\tN.TRUNC\tN.ZERO\tLLK.OBS\tLLK.EXP\tLLK.SD\tZ\tP\tZ.SNG1\tFLAG\n"
DONORS_HEADER = "SM_ID\tN.CELL\tMED.Z\tMIN.Z\tN.MISFIT\tFRAC.MISFIT\n"


@dataclass
class BestHyp:
    """Every row of a `.best` by cell id (hyp = (-1, -1) and best = "" without a row)."""
    best: list               # BEST strings
    hyp: np.ndarray          # int32 [B][2]: (v1, -1) singlet, (v1, v2) doublet
    alpha: np.ndarray        # float64 [B]: the doublet's share of v2, 0 for singlets
    sng1: np.ndarray         # int32 [B]: SNG.1ST

    @property
    def has_row(self) -> np.ndarray:
        return self.hyp[:, 0] >= 0


def hypothesis_of_row(best: str, sng1: int, llk_sng1: float, dbl1: int, dbl2: int, alpha: float, llk12: float):
    """(v1, v2, alpha) of one `.best` row: SNG- is (SNG.1ST, -1, 0); DBL- is (DBL.1ST, DBL.2ND, ALPHA); AMB- the one of the two with the
    larger LLK of the row itself (the singlet on a tie).  A doublet whose two samples coincide, or whose share is 0, is the singlet."""
    if best.startswith("SNG-"):
        return sng1, -1, 0.0
    if not (best.startswith("DBL-") or best.startswith("AMB-")):
        raise ValueError(f"BEST {best!r} is not SNG-, DBL- or AMB-")
    dbl_ok = dbl1 >= 0 and dbl2 >= 0 and dbl1 != dbl2
    if best.startswith("AMB-") and not (dbl_ok and llk12 > llk_sng1):
        return sng1, -1, 0.0
    if not dbl_ok:
        return sng1, -1, 0.0
    return dbl1, dbl2, alpha


def read_best_hypotheses(path: str, sample_ids: Sequence[str], barcodes: Sequence[str]) -> BestHyp:
    smap = {s: j for j, s in enumerate(sample_ids)}
    cmap = {b: c for c, b in enumerate(barcodes)}
    B = len(barcodes)
    out = BestHyp([""] * B, np.full((B, 2), -1, dtype=np.int32), np.zeros(B), np.full(B, -1, dtype=np.int32))
    need = ("BARCODE", "BEST", "SNG.1ST", "SNG.LLK1", "DBL.1ST", "DBL.2ND", "ALPHA", "LLK12")
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        col = {n: i for i, n in enumerate(head)}
        for n in need:
            if n not in col:
                raise ValueError(f"{path}: no {n} column")
        for line in f:
            t = line.rstrip("\n").split("\t")
            if len(t) < len(head):
                continue
            c = cmap.get(t[col["BARCODE"]])
            if c is None:
                raise ValueError(f"{path}: barcode {t[col['BARCODE']]!r} not in this job")
            idx = []
            for n in ("SNG.1ST", "DBL.1ST", "DBL.2ND"):
                j = smap.get(t[col[n]])
                if j is None:
                    raise ValueError(f"{path}: sample {t[col[n]]!r} not in this job")
                idx.append(j)
            al = float(t[col["ALPHA"]])
            if not 0.0 <= al <= 1.0:
                raise ValueError(f"{path}: ALPHA {al} of {t[col['BARCODE']]!r} is not in [0, 1]")
            v1, v2, a = hypothesis_of_row(t[col["BEST"]], idx[0], float(t[col["SNG.LLK1"]]), idx[1], idx[2], al, float(t[col["LLK12"]]))
            out.best[c] = t[col["BEST"]]
            out.hyp[c] = (v1, v2)
            out.alpha[c] = a if v2 >= 0 else 0.0
            out.sng1[c] = idx[0]
    return out


def hypothesis_label(v1: int, v2: int, alpha: float, sample_ids: Sequence[str]) -> str:
    if v2 < 0:
        return f"SNG-{sample_ids[int(v1)]}"
    return f"DBL-{sample_ids[int(v1)]}-{sample_ids[int(v2)]}-{alpha:.3f}"


def z_scores(obs, mean, var) -> np.ndarray:
    """Z = (obs - mean) / sqrt(var); nan where var is 0 (or not a positive finite number)."""
    obs, mean, var = (np.asarray(x, dtype=np.float64) for x in (obs, mean, var))
    ok = np.isfinite(var) & (var > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok, (obs - mean) / np.sqrt(np.where(ok, var, 1.0)), np.nan)


def lower_tail(z) -> np.ndarray:
    """P = erfc(-Z / sqrt 2) / 2."""
    return np.array([0.5 * math.erfc(-float(x) / math.sqrt(2.0)) if np.isfinite(x) else np.nan for x in np.asarray(z, dtype=np.float64)])


def read_rho_tsv(path: str, barcodes: Sequence[str]) -> np.ndarray:
    """rho[cell id] from the BARCODE and RHO columns of an ambient.py `.ambient.tsv`; 0 for barcodes it does not list."""
    cmap = {b: c for c, b in enumerate(barcodes)}
    rho = np.zeros(len(barcodes))
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        col = {n: i for i, n in enumerate(head)}
        for n in ("BARCODE", "RHO"):
            if n not in col:
                raise ValueError(f"{path}: no {n} column")
        for line in f:
            t = line.rstrip("\n").split("\t")
            if len(t) < len(head) or t[0].startswith("#"):
                continue
            c = cmap.get(t[col["BARCODE"]])
            if c is None:
                raise ValueError(f"{path}: barcode {t[col['BARCODE']]!r} not in this job")
            r = float(t[col["RHO"]])
            if not 0.0 <= r <= 1.0:
                raise ValueError(f"{path}: RHO {r} of {t[col['BARCODE']]!r} is not in [0, 1]")
            rho[c] = r
    return rho


def _num(x, fmt: str) -> str:
    return format(float(x), fmt) if np.isfinite(x) else "NA"


def write_fit_tsv(path: str, barcodes: Sequence[str], sample_ids: Sequence[str], rows: BestHyp, r: dict, z, p, z_sng1, z_min: float) -> int:
    """One row per barcode of the `.best`, in ascending byte-wise barcode order (the writers' order); returns the number of MISFIT rows."""
    order = sorted(np.flatnonzero(rows.has_row), key=lambda k: barcodes[k].encode())
    n_flag = 0
    with open(path, "w") as f:
        f.write(FIT_HEADER)
        for k in order:
            sd = math.sqrt(r["var"][k]) if np.isfinite(r["var"][k]) and r["var"][k] > 0.0 else 0.0
            flag = "MISFIT" if np.isfinite(z[k]) and z[k] < z_min else "."
            n_flag += flag == "MISFIT"
            f.write(f"{barcodes[k]}\t{rows.best[k]}\t{hypothesis_label(rows.hyp[k, 0], rows.hyp[k, 1], rows.alpha[k], sample_ids)}\t{int(r['n_snp'][k])}\t"
                    f"{int(r['n_read'][k])}\t{int(r['n_trunc'][k])}\t{int(r['n_zero'][k])}\t{_num(r['obs'][k], '.5f')}\t{_num(r['mean'][k], '.5f')}\t"
                    f"{sd:.5f}\t{_num(z[k], '.4f')}\t{_num(p[k], '.4g')}\t{_num(z_sng1[k], '.4f')}\t{flag}\n")
    return n_flag


def donor_summary(rows: BestHyp, z, z_min: float, n_samples: int):
    """[(label index, N.CELL, MED.Z, MIN.Z, N.MISFIT)]: index v < n_samples over the singlet hypotheses of sample v, n_samples for the doublet
    hypotheses, n_samples + 1 for the pool.  MED.Z / MIN.Z over the barcodes with a Z (nan without one)."""
    z = np.asarray(z, dtype=np.float64)
    sng = rows.has_row & (rows.hyp[:, 1] < 0)
    groups = [sng & (rows.hyp[:, 0] == v) for v in range(n_samples)] + [rows.has_row & (rows.hyp[:, 1] >= 0), rows.has_row]
    out = []
    for i, m in enumerate(groups):
        zz = z[m & np.isfinite(z)]
        out.append((i, int(m.sum()), float(np.median(zz)) if len(zz) else np.nan, float(zz.min()) if len(zz) else np.nan, int((zz < z_min).sum())))
    return out


def write_donors_tsv(path: str, sample_ids: Sequence[str], summary) -> None:
    V = len(sample_ids)
    with open(path, "w") as f:
        f.write(DONORS_HEADER)
        for i, n, med, mn, k in summary:
            name = sample_ids[i] if i < V else ("DBL" if i == V else "#POOL")
            f.write(f"{name}\t{n}\t{_num(med, '.4f')}\t{_num(mn, '.4f')}\t{k}\t{_num(k / n if n else np.nan, '.4f')}\n")


def fit_run(store_or_pileup, g: np.ndarray, sample_ids: Sequence[str], out_prefix: str, best: Optional[str] = None, max_reads: int = 4,
            z_min: float = -4.0, rho=None, ambient="reads", alphas: Sequence[float] = (0.0, 0.5), barcodes: Optional[Sequence[str]] = None,
            device: int = 0, mode: int = capi.DMX_MODE_STRICT, **demuxlet_run_kwargs):
    """Score every barcode of `best` (a `.best` path) under its own call against genotype matrix g.  Without `best`, the unchanged
    demuxlet_run writes <out_prefix>.best/.single/.sing2 first.  `rho` (None = no soup) is a per-barcode soup fraction [B]; `ambient` is
    then "reads", "genotypes", "census" or an array of n_snps ALT frequencies.  `store_or_pileup` is a Store, or a HostPileup with
    barcodes=... as for demuxlet_run.  Writes <out_prefix>.fit.tsv and .fit_donors.tsv; returns a dict with the rows, both engine results,
    Z, P, Z.SNG1, the flags and the donor summary."""
    from . import ambient as amb_mod
    g = np.ascontiguousarray(g, dtype=np.float32)
    if not 1 <= int(max_reads) <= MAX_READS:
        raise ValueError(f"max_reads: 1 to {MAX_READS}, not {max_reads}")
    if not np.isfinite(z_min):
        raise ValueError("z_min must be finite")
    if isinstance(ambient, str) and ambient not in ("reads", "genotypes", "census"):
        raise ValueError(f"ambient: 'reads', 'genotypes', 'census' or an array, not {ambient!r}")
    if isinstance(store_or_pileup, engine.HostPileup):
        pl = store_or_pileup
        if barcodes is None:
            raise ValueError("fit_run: a HostPileup needs barcodes=")
    else:
        pl, barcodes = store_or_pileup.freeze(), store_or_pileup.barcodes()
    if g.ndim != 3 or g.shape[0] != pl.n_snps or g.shape[1] != len(sample_ids) or g.shape[2] != 3:
        raise ValueError(f"genotype matrix {g.shape} for {pl.n_snps} SNPs and {len(sample_ids)} samples")
    if rho is not None:
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        if rho.shape != (pl.n_cells,) or not np.all((rho >= 0.0) & (rho <= 1.0)):
            raise ValueError(f"rho: {pl.n_cells} values in [0, 1]")
        if not isinstance(ambient, str):
            ambient = amb_mod.check_ambient(ambient, pl.n_snps)
    if best is None:
        engine.demuxlet_run(pl, g, sample_ids, alphas, out_prefix, barcodes=barcodes, device=device, mode=mode, **demuxlet_run_kwargs)
        best = out_prefix + ".best"
    rows = read_best_hypotheses(best, sample_ids, barcodes)
    other = rows.has_row & np.array([not b.startswith("SNG-") for b in rows.best])
    hyp1 = np.full_like(rows.hyp, -1)
    hyp1[other, 0] = rows.sng1[other]
    eng = engine.Engine(len(sample_ids), alphas, device=device, mode=mode)
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        a = None
        if rho is not None:
            a = amb_mod._ambient_builder(ambient, eng, g, lambda: refine.assignments_from_best(best, sample_ids, barcodes)) if isinstance(ambient, str) else ambient
        r = eng.fit_profile(rows.hyp, rows.alpha, rho, a, max_reads)
        info = eng.fit_info()
        r1 = eng.fit_profile(hyp1, np.zeros(pl.n_cells), rho, a, max_reads)
    finally:
        eng.close()
    z = z_scores(r["obs"], r["mean"], r["var"])
    z1 = np.where(other, z_scores(r1["obs"], r1["mean"], r1["var"]), z)
    p = lower_tail(z)
    n_flag = write_fit_tsv(out_prefix + ".fit.tsv", barcodes, sample_ids, rows, r, z, p, z1, z_min)
    summary = donor_summary(rows, z, z_min, len(sample_ids))
    write_donors_tsv(out_prefix + ".fit_donors.tsv", sample_ids, summary)
    with np.errstate(invalid="ignore"):
        flag = rows.has_row & (z < z_min)
    return dict(rows=rows, fit=r, fit_sng1=r1, info=info, z=z, p=p, z_sng1=z1, flag=flag, n_misfit=n_flag, donors=summary, ambient=a)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.fit", description="goodness of fit of every call: flag droplets that no donor explains")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.fit.tsv, <out>.fit_donors.tsv (and <out>.best/... without --best)")
    ap.add_argument("--best", help="a .best of this pileup: its calls are the hypotheses (default: run the demultiplexing pass first)")
    ap.add_argument("--max-reads", type=int, default=4, help=f"reads of a (barcode, SNP) pair that enter, 1..{MAX_READS} (default 4)")
    ap.add_argument("--z-min", type=float, default=-4.0, help="FLAG is MISFIT below this Z (default -4: a one-sided 3e-5)")
    ap.add_argument("--ambient-tsv", help="<x>.ambient.tsv of an ambient.py run: its RHO per barcode is the soup fraction of the hypothesis")
    ap.add_argument("--ambient", choices=("reads", "genotypes", "census"), default=None,
                    help="soup ALT frequency, as for ambient.py (default reads); needs --ambient-tsv")
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.0, 0.5], help="doublet grid of the demultiplexing pass (default 0 0.5)")
    ap.add_argument("--fast", action="store_true", help="DMX_MODE_FAST for the demultiplexing pass")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    if not 1 <= a.max_reads <= MAX_READS:
        ap.error(f"--max-reads must be in [1, {MAX_READS}]")
    if not np.isfinite(a.z_min):
        ap.error("--z-min must be finite")
    if a.ambient is not None and a.ambient_tsv is None:
        ap.error("--ambient needs --ambient-tsv")
    if a.ambient is None:
        a.ambient = "reads"
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    d = refine.read_pileup_txt(a.pileup)
    rho = read_rho_tsv(a.ambient_tsv, d.barcodes) if a.ambient_tsv else None
    r = fit_run(d.pileup, d.g, d.sample_ids, a.out, best=a.best, max_reads=a.max_reads, z_min=a.z_min, rho=rho, ambient=a.ambient,
                alphas=a.alpha, barcodes=d.barcodes, device=a.gpu, mode=capi.DMX_MODE_FAST if a.fast else capi.DMX_MODE_STRICT)
    print(f"{int(r['rows'].has_row.sum())} barcodes scored; {r['n_misfit']} MISFIT (Z < {a.z_min:g})", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
