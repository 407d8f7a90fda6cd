"""Empirical-Bayes priors: the donors' shares of the pool's cells and the doublet rate, fitted from the doublet grid, and every
barcode's posterior under them.

The reference's posteriors put the same weight 1 / V on every donor and take a doublet prior the user has to guess.  Here a droplet
holds two cells with probability d, otherwise one; cells are independent draws from the donor shares pi; a homotypic doublet looks like
its singlet; a doublet's mixing share is uniform over the grid's alphas.  The engine fits (pi, d) by EM over the grid llksAB that the
doublet stage leaves on the device (Engine.prior_fit, dmx_engine_prior_fit) and evaluates the per-barcode record
at the fit (Engine.prior_call).  The reference's own calls are not touched.

    python -m demuxlet_amd.prior --pileup <x>.pileup.txt --out <prefix> [--alpha A ...] [--max-iter 200] [--tol 1e-6] [--fix-shares]
        [--fix-rate D] [--min-post 0.9] [--min-total/--min-uniq/--min-snp N] [--fast] [--gpu G]

reads the dump that `demuxlet --pileup-only` writes, runs the unchanged pipeline (<prefix>.best/.single/.sing2 as every front end
writes them) and then writes

  <prefix>.prior.tsv      SM_ID SHARE N.CELL — one row per donor; N.CELL = the expected number of the donor's cells among the fitted
                          barcodes; then a trailer of `#NAME<TAB>value` lines: RATE.DBL (d), RATE.HET (d (1 - sum pi^2)), N.HOM (the
                          expected homotypic doublets), N.BARCODE, LLK, ITER, CONVERGED
  <prefix>.prior_fit.tsv  ITER LLK RATE.DBL — the log-likelihood of every iteration and the rate it was evaluated at
  <prefix>.eb.tsv         BARCODE N.SNP BEST CALL PRB.SNG PRB.HET PRB.HOM SNG.1ST PRB.SNG1 SNG.2ND PRB.SNG2 DBL.1ST DBL.2ND ALPHA PRB.DBL1
                          LLK.EVID — one row per barcode of the `.best`, in its order.  BEST is the reference's call.  CALL is
                          DBL-a-b-alpha when PRB.HET >= --min-post (a before b in VCF order at alpha = 0.5), SNG-j when PRB.SNG1 >=
                          --min-post, otherwise AMB-j1-j2-a/b in the reference's shape; DBL.1ST / DBL.2ND are printed in CALL's order.  PRB.SNG1 counts a homotypic doublet of j with j:
                          no genotype method can tell them apart; PRB.HOM says how much of the barcode's mass that is."""
from __future__ import annotations

import argparse
import sys
from typing import Optional, Sequence

import numpy as np

from . import ambient, capi, engine, refine

PRIOR_HEADER = "SM_ID\tSHARE\tN.CELL\n"
FIT_HEADER = "ITER\tLLK\tRATE.DBL\n"
EB_HEADER = ("BARCODE\tN.SNP\tBEST\tCALL\tPRB.SNG\tPRB.HET\tPRB.HOM\tSNG.1ST\tPRB.SNG1\tSNG.2ND\tPRB.SNG2\tDBL.1ST\tDBL.2ND\tALPHA\tPRB.DBL1\t"
             "LLK.EVID\n")


def uniform_rate(doublet_prior: float, V: int) -> float:
    """The d at which uniform shares give the reference's posterior PRB.DBL for --doublet-prior p on a grid whose alphas above 0 are all
    0.5: d = t V / (1 + t (V - 1)), t = p / (2 (V - 1) (1 - p))."""
    if doublet_prior >= 1.0:
        return 1.0
    t = doublet_prior / (2.0 * (V - 1) * (1.0 - doublet_prior))
    return t * V / (1.0 + t * (V - 1))


def dbl_pair(rec, alphas):
    """(a, b, alpha) of a record's largest doublet term as it is printed: a before b in VCF order at alpha = 0.5, where the two orders
    are one hypothesis; (-1, -1, 0.0) without one."""
    a, b = int(rec["j_dbl"]), int(rec["k_dbl"])
    al = float(alphas[int(rec["n_dbl"])]) if rec["n_dbl"] >= 0 else 0.0
    if a >= 0 and al == 0.5 and a > b:
        a, b = b, a
    return a, b, al


def eb_call(rec, alphas, sample_ids: Sequence[str], min_post: float) -> str:
    """CALL of one record (a row of Engine.prior_call's array)."""
    name = lambda j: sample_ids[int(j)] if j >= 0 else "."
    a, b, al = dbl_pair(rec, alphas)
    if rec["p_het"] >= min_post:
        return f"DBL-{name(a)}-{name(b)}-{al:.3f}"
    if rec["p_sng1"] >= min_post:
        return f"SNG-{name(rec['i_sng1'])}"
    return f"AMB-{name(rec['i_sng1'])}-{name(rec['i_sng2'])}-{name(a)}/{name(b)}"


def write_prior_tsv(path: str, sample_ids: Sequence[str], fit: dict) -> None:
    pi, d = fit["pi"], fit["d"]
    n_cell = fit["N"]
    with open(path, "w") as f:
        f.write(PRIOR_HEADER)
        for j, s in enumerate(sample_ids):
            f.write(f"{s}\t{pi[j]:.6f}\t{n_cell[j]:.2f}\n")
        f.write(f"#RATE.DBL\t{d:.6f}\n#RATE.HET\t{d * (1.0 - float(np.sum(pi * pi))):.6f}\n#N.HOM\t{fit['hom']:.2f}\n#N.BARCODE\t{fit['b_in']}\n"
                f"#LLK\t{fit['ll']:.5f}\n#ITER\t{fit['n_iter']}\n#CONVERGED\t{int(fit['converged'])}\n")


def write_fit_tsv(path: str, fit: dict) -> None:
    with open(path, "w") as f:
        f.write(FIT_HEADER)
        for it in range(fit["n_iter"]):
            f.write(f"{it}\t{fit['ll_trace'][it]:.5f}\t{fit['d_trace'][it]:.6f}\n")


def write_eb_tsv(path: str, order: Sequence[int], barcodes: Sequence[str], sample_ids: Sequence[str], best: Sequence[str], n_snp, rec, alphas,
                 min_post: float) -> None:
    name = lambda j: sample_ids[int(j)] if j >= 0 else "."
    with open(path, "w") as f:
        f.write(EB_HEADER)
        for k in order:
            r = rec[k]
            a, b, alpha = dbl_pair(r, alphas)          # DBL.1ST / DBL.2ND in CALL's order
            al = f"{alpha:.3f}" if a >= 0 else "."
            f.write(f"{barcodes[k]}\t{int(n_snp[k])}\t{best[k]}\t{eb_call(r, alphas, sample_ids, min_post)}\t{r['p_sng']:.5f}\t{r['p_het']:.5f}\t"
                    f"{r['p_hom']:.5f}\t{name(r['i_sng1'])}\t{r['p_sng1']:.5f}\t{name(r['i_sng2'])}\t{r['p_sng2']:.5f}\t{name(a)}\t"
                    f"{name(b)}\t{al}\t{r['p_dbl1']:.5f}\t{r['log_e']:.5f}\n")


def prior_run(store_or_pileup, g: np.ndarray, sample_ids: Sequence[str], out_prefix: str, alphas: Sequence[float] = (0.0, 0.5),
              max_iter: int = 200, tol: float = 1e-6, fix_shares: bool = False, fix_rate: Optional[float] = None, min_post: float = 0.9,
              d0: float = 0.1, barcodes: Optional[Sequence[str]] = None, device: int = 0, mode: int = capi.DMX_MODE_STRICT,
              **demuxlet_run_kwargs) -> dict:
    """The unchanged demuxlet_run first (<out_prefix>.best/.single/.sing2), then the fit of (pi, d) over the barcodes of the `.best` and
    the records at the fit.  fix_shares holds pi uniform; fix_rate=D holds d at D.  `store_or_pileup` is a Store, or a HostPileup with
    barcodes=.  Writes the three files of the module's docstring; returns a dict: fit (Engine.prior_fit's), calls (Engine.prior_call's
    array by cell id), rows (the `.best` rows), mask, order (the `.best`'s cell ids in its order), info."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    if isinstance(store_or_pileup, engine.HostPileup):
        pl = store_or_pileup
        if barcodes is None:
            raise ValueError("prior_run: a HostPileup needs barcodes=")
    else:
        pl, barcodes = store_or_pileup.freeze(), store_or_pileup.barcodes()
    V = len(sample_ids)
    if g.ndim != 3 or g.shape[0] != pl.n_snps or g.shape[1] != V or g.shape[2] != 3:
        raise ValueError(f"genotype matrix {g.shape} for {pl.n_snps} SNPs and {V} samples")
    if V < 2 or len(alphas) < 2:
        raise ValueError("prior_run: at least two samples and two alphas needed")
    if fix_rate is not None and not 0.0 <= fix_rate <= 1.0:
        raise ValueError("prior_run: fix_rate must be in [0, 1]")
    if not 0.0 < min_post <= 1.0:
        raise ValueError("prior_run: min_post must be in (0, 1]")
    engine.demuxlet_run(pl, g, sample_ids, alphas, out_prefix, barcodes=barcodes, device=device, mode=mode, **demuxlet_run_kwargs)
    rows = ambient.read_best_rows(out_prefix + ".best", sample_ids, barcodes)
    n_snp = np.asarray(pl.n_snp_per_cell)
    mask = rows.has_row & (n_snp > 0)
    if not mask.any():
        raise ValueError("prior_run: the .best has no barcode with a SNP")
    eng = engine.Engine(V, alphas, device=device, mode=mode)
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        eng.run_doublet()
        fit = eng.prior_fit(mask=mask, d0=d0 if fix_rate is None else fix_rate, max_iter=max_iter, tol=tol, fix_pi=fix_shares,
                            fix_d=fix_rate is not None)
        info = eng.prior_info()
        rec = eng.prior_call(fit["pi"], fit["d"], mask=mask)
        info["call_ms"] = eng.prior_info()["call_ms"]
    finally:
        eng.close()
    order = sorted(np.flatnonzero(mask), key=lambda k: barcodes[k].encode())
    write_prior_tsv(out_prefix + ".prior.tsv", sample_ids, fit)
    write_fit_tsv(out_prefix + ".prior_fit.tsv", fit)
    write_eb_tsv(out_prefix + ".eb.tsv", order, barcodes, sample_ids, rows.best, n_snp, rec, eng.alphas, min_post)
    return dict(fit=fit, calls=rec, rows=rows, mask=mask, order=order, info=info)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.prior", description="empirical-Bayes donor shares and doublet rate of a pool")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.prior.tsv, <out>.prior_fit.tsv, <out>.eb.tsv (and <out>.best/...)")
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.0, 0.5], help="doublet grid (default 0 0.5)")
    ap.add_argument("--max-iter", type=int, default=200, help="EM iterations at most (default 200)")
    ap.add_argument("--tol", type=float, default=1e-6, help="stop once an iteration gains less than this per barcode in log-likelihood (default 1e-6)")
    ap.add_argument("--fix-shares", action="store_true", help="hold the shares uniform and fit the rate alone")
    ap.add_argument("--fix-rate", type=float, metavar="D", help="hold the doublet rate at D and fit the shares alone")
    ap.add_argument("--min-post", type=float, default=0.9, help="posterior a DBL or SNG call needs (default 0.9)")
    ap.add_argument("--min-total", type=int, default=0)
    ap.add_argument("--min-uniq", type=int, default=0)
    ap.add_argument("--min-snp", type=int, default=0)
    ap.add_argument("--fast", action="store_true", help="DMX_MODE_FAST")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    if len(a.alpha) < 2:
        ap.error("--alpha needs at least two values")
    if a.max_iter < 1:
        ap.error("--max-iter must be >= 1")
    if not a.tol > 0.0:
        ap.error("--tol must be > 0")
    if a.fix_rate is not None and not 0.0 <= a.fix_rate <= 1.0:
        ap.error("--fix-rate must be in [0, 1]")
    if not 0.0 < a.min_post <= 1.0:
        ap.error("--min-post must be in (0, 1]")
    if a.gpu < 0:
        ap.error("--gpu must be >= 0")
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    d = refine.read_pileup_txt(a.pileup)
    r = prior_run(d.pileup, d.g, d.sample_ids, a.out, alphas=a.alpha, max_iter=a.max_iter, tol=a.tol, fix_shares=a.fix_shares,
                  fix_rate=a.fix_rate, min_post=a.min_post, barcodes=d.barcodes, device=a.gpu,
                  mode=capi.DMX_MODE_FAST if a.fast else capi.DMX_MODE_STRICT, min_total=a.min_total, min_uniq=a.min_uniq, min_snp=a.min_snp)
    f = r["fit"]
    top = int(np.argmax(f["pi"]))
    print(f"prior: {f['b_in']} barcodes, {f['n_iter']} iterations{'' if f['converged'] else ' (not converged)'}, doublet rate {f['d']:.4f}; "
          f"largest share {d.sample_ids[top]} {f['pi'][top]:.4f}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
