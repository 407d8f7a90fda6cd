"""What do the calls and the fit statistics do on a pool where the model holds exactly?  Model-drawn null pools.

    python -m demuxlet_amd.redraw --pileup <x>.pileup.txt --out <prefix> [--best <x>.best] [--reps 20] [--genotype-draw donor|pair]
        [--seed S] [--geno-seed S] [--max-reads 4] [--min-cells 10] [--fpr 0.001] [--singlets-only]
        [--ambient-tsv <x>.ambient.tsv [--ambient reads|genotypes|census]] [--alpha A ...] [--fast] [--gpu G]

The parametric bootstrap of a pool.  The real pool's structure is kept — which barcode covers which SNP, with how many reads, at which
base qualities — and every read's allele is drawn again on the GPU from the model under the barcode's own call (Engine.redraw,
dmx_engine_redraw).  In such a pool the truth is known and the model holds exactly: whatever fit.py's and sites.py's
Z do there is their null law at this pool's depth, and whatever the plain pass miscalls there is its error rate.

Each barcode's hypothesis is its BEST call (fit.read_best_hypotheses; --singlets-only leaves the doublet calls out), with RHO per barcode
from --ambient-tsv.  On the real pool fit_profile and site_fit give the observed Z per barcode and per SNP.  Then, for every replicate,
the pool is redrawn (barcode b of replicate r is hashed as r B + b), a second engine adopts the redrawn pileup where it lies, the
unchanged demultiplexing pass calls it, and fit_profile and site_fit score it under the TRUE hypotheses.

  --genotype-draw donor   (default) a donor has ONE genotype per SNP, drawn from its row, in every barcode and every replicate — as in a
                          real pool.  With soft rows the cells of a donor share that genotype, which the site audit's summed per-pair
                          variance does not know: the null pool shows by how much.  The honest mode for sites.
  --genotype-draw pair    a genotype per (barcode, SNP) pair: exactly the law under which fit.py's mean and variance are computed.

  <prefix>.null.best          the last replicate's calls, in the ordinary format (.null.single / .null.sing2 beside it)
  <prefix>.null.tsv           REP BARCODE TRUTH BEST OK Z — one row per replicate and barcode with a hypothesis; OK as simulate.py counts it
  <prefix>.null_fit.tsv       BARCODE HYP Z.OBS NULL.MEAN NULL.SD P.EMP, P.EMP = (1 + #{null Z <= Z.OBS}) / (reps + 1)
  <prefix>.null_sites.tsv     SNP N.CELL and the same four columns for Z and for Z.ALT
  <prefix>.null_summary.tsv   per truth kind (SNG, DBL): N, N.OK, singlets called DBL, doublets called SNG, wrong donor, AMB; then the
                              pooled null Z of the barcodes and of the SNPs with N.CELL >= --min-cells: N, mean, sd and the --fpr
                              quantile — the values to pass as fit.py --z-min and sites.py --z-min

Limits.  The hypotheses are calls, and the null pool is drawn from them: a miscalled barcode is redrawn as what it was called.  Nothing is
fitted.  share.py's LLR, the triplet and the prior passes are not calibrated here; no `.pair` output; one GPU."""
from __future__ import annotations

import argparse
import sys
from typing import Optional, Sequence

import numpy as np

from . import ambient as amb_mod
from . import capi, engine, fit, refine, simulate, sites

NULL_HEADER = "REP\tBARCODE\tTRUTH\tBEST\tOK\tZ\n"
NULL_FIT_HEADER = "BARCODE\tHYP\tZ.OBS\tNULL.MEAN\tNULL.SD\tP.EMP\n"
NULL_SITES_HEADER = "SNP\tN.CELL\tZ.OBS\tNULL.MEAN\tNULL.SD\tP.EMP\tZ.ALT.OBS\tZ.ALT.NULL.MEAN\tZ.ALT.NULL.SD\tZ.ALT.P.EMP\n"
SUMMARY_HEADER = "KIND\tN\tN.OK\tSNG.AS.DBL\tDBL.AS.SNG\tN.WRONG\tN.AMB\n"
POOLED_HEADER = "#NULL\tN\tMEAN\tSD\tQUANTILE\tFPR\n"
DRAWS = ("donor", "pair")


def check_args(reps: int, fpr: float, min_cells: int, max_reads: int, genotype_draw: str, seed: int = 0, geno_seed: int = 0) -> None:
    if int(reps) < 1:
        raise ValueError(f"reps: at least 1, not {reps}")
    if not 0.0 < float(fpr) < 1.0:
        raise ValueError(f"fpr must be in (0, 1), not {fpr}")
    if int(min_cells) < 0:
        raise ValueError("min_cells must not be negative")
    if not 1 <= int(max_reads) <= fit.MAX_READS:
        raise ValueError(f"max_reads: 1 to {fit.MAX_READS}, not {max_reads}")
    if genotype_draw not in DRAWS:
        raise ValueError(f"genotype_draw: 'donor' or 'pair', not {genotype_draw!r}")
    if int(seed) < 0 or int(geno_seed) < 0:
        raise ValueError("seed and geno_seed must not be negative")


def p_emp(z_obs, null_z) -> np.ndarray:
    """P.EMP[k] = (1 + #{r: null_z[r][k] <= z_obs[k]}) / (reps + 1); a null Z that is not a number never counts as below, and an
    observed Z that is not a number has no P.EMP (nan)."""
    z = np.asarray(z_obs, dtype=np.float64)
    nz = np.asarray(null_z, dtype=np.float64).reshape(-1, len(z))
    with np.errstate(invalid="ignore"):
        below = (nz <= z[None, :]).sum(axis=0)
    return np.where(np.isnan(z), np.nan, (1.0 + below) / (nz.shape[0] + 1.0))


def null_moments(null_z):
    """(mean, sd) per column over the replicates whose Z is a number (nan without one; sd with the divisor n)."""
    nz = np.asarray(null_z, dtype=np.float64)
    ok = np.isfinite(nz)
    n = ok.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(ok, nz, 0.0).sum(axis=0) / n
        sd = np.sqrt(np.where(ok, (nz - mean[None, :]) ** 2, 0.0).sum(axis=0) / n)
    return np.where(n > 0, mean, np.nan), np.where(n > 0, sd, np.nan)


def pooled_null(values, fpr: float) -> dict:
    """N, mean, sd (divisor n) and the lower fpr quantile of the finite entries of `values`."""
    v = np.asarray(values, dtype=np.float64).ravel()
    v = v[np.isfinite(v)]
    if not len(v):
        return dict(n=0, mean=np.nan, sd=np.nan, quantile=np.nan)
    return dict(n=int(len(v)), mean=float(v.mean()), sd=float(v.std()), quantile=float(np.quantile(v, fpr)))


def truth_ok(v1: int, v2: int, best: str, sng1: int, dbl1: int, dbl2: int) -> bool:
    """simulate.row_ok for a barcode whose truth is hyp = (v1, v2): a doublet must be called DBL- with its two donors, a singlet SNG- of its donor."""
    return bool(best) and simulate.row_ok(simulate.KIND_HET if v2 >= 0 else simulate.KIND_SNG, (v1, v2), best, sng1, dbl1, dbl2)


def summary_counts(hyp, best: Sequence[str], sng1, dbl1, dbl2) -> dict:
    """Per truth kind ("SNG", "DBL"): n, n_ok, as_dbl (singlets called DBL-), as_sng (doublets called SNG-), wrong (the right kind of call
    with a wrong donor), amb (AMB- or no row).  n = n_ok + the four others of its kind.  Unused barcodes (v1 < 0) are not counted."""
    out = {k: dict(n=0, n_ok=0, as_dbl=0, as_sng=0, wrong=0, amb=0) for k in ("SNG", "DBL")}
    hyp = np.asarray(hyp).reshape(-1, 2)
    for k in range(len(hyp)):
        v1, v2 = int(hyp[k, 0]), int(hyp[k, 1])
        if v1 < 0:
            continue
        t = out["DBL" if v2 >= 0 else "SNG"]
        t["n"] += 1
        b = best[k]
        if truth_ok(v1, v2, b, int(sng1[k]), int(dbl1[k]), int(dbl2[k])):
            t["n_ok"] += 1
        elif b.startswith("DBL-"):
            t["wrong" if v2 >= 0 else "as_dbl"] += 1
        elif b.startswith("SNG-"):
            t["as_sng" if v2 >= 0 else "wrong"] += 1
        else:
            t["amb"] += 1
    return out


def add_counts(total: dict, part: dict) -> None:
    for kind in total:
        for k in total[kind]:
            total[kind][k] += part[kind][k]


def write_summary_tsv(path: str, counts: dict, pooled_fit: dict, pooled_sites: dict, fpr: float) -> None:
    num = fit._num
    with open(path, "w") as f:
        f.write(SUMMARY_HEADER)
        for kind in ("SNG", "DBL"):
            c = counts[kind]
            f.write(f"{kind}\t{c['n']}\t{c['n_ok']}\t{c['as_dbl']}\t{c['as_sng']}\t{c['wrong']}\t{c['amb']}\n")
        f.write(POOLED_HEADER)
        for name, p in (("#NULL.FIT", pooled_fit), ("#NULL.SITES", pooled_sites)):
            f.write(f"{name}\t{p['n']}\t{num(p['mean'], '.6f')}\t{num(p['sd'], '.6f')}\t{num(p['quantile'], '.4f')}\t{fpr:g}\n")


def redraw_run(pileup: engine.HostPileup, g: np.ndarray, sample_ids: Sequence[str], out_prefix: str, barcodes: Sequence[str],
               best: Optional[str] = None, reps: int = 20, genotype_draw: str = "donor", seed: int = 0, geno_seed: int = 0, max_reads: int = 4,
               min_cells: int = 10, fpr: float = 0.001, singlets_only: bool = False, rho=None, ambient="reads",
               alphas: Sequence[float] = (0.0, 0.5), device: int = 0, mode: int = capi.DMX_MODE_STRICT, **demuxlet_run_kwargs) -> dict:
    """Calibrate the calls and both fit statistics of `pileup` on `reps` model-drawn null pools and write the five files named in the module
    docstring.  Without `best` the unchanged demuxlet_run writes <out_prefix>.best/.single/.sing2 first.  `rho` / `ambient` as for
    fit.fit_run.  Returns a dict with the hypotheses, the observed and the null Z (barcodes, sites, Z.ALT), P.EMP, the call counts, the
    pooled moments and the redraw kernel's total time."""
    check_args(reps, fpr, min_cells, max_reads, genotype_draw, seed, geno_seed)
    g = np.ascontiguousarray(g, dtype=np.float32)
    pl = pileup
    B, S = pl.n_cells, pl.n_snps
    if g.ndim != 3 or g.shape[0] != S or g.shape[1] != len(sample_ids) or g.shape[2] != 3:
        raise ValueError(f"genotype matrix {g.shape} for {S} SNPs and {len(sample_ids)} samples")
    if isinstance(ambient, str) and ambient not in ("reads", "genotypes", "census"):
        raise ValueError(f"ambient: 'reads', 'genotypes', 'census' or an array, not {ambient!r}")
    if rho is not None:
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        if rho.shape != (B,) or not np.all((rho >= 0.0) & (rho <= 1.0)):
            raise ValueError(f"rho: {B} values in [0, 1]")
        if not isinstance(ambient, str):
            ambient = amb_mod.check_ambient(ambient, S)
    if best is None:
        engine.demuxlet_run(pl, g, sample_ids, alphas, out_prefix, barcodes=barcodes, device=device, mode=mode, **demuxlet_run_kwargs)
        best = out_prefix + ".best"
    rows = fit.read_best_hypotheses(best, sample_ids, barcodes)
    hyp, alpha = sites.hypotheses(rows, singlets_only)
    used = hyp[:, 0] >= 0
    src = pl.as_struct()                             # (makes the rd_* counters contiguous int32: they are attached to every redrawn view)
    null_prefix = out_prefix + ".null"
    null_fit = np.full((reps, B), np.nan); null_site = np.full((reps, S), np.nan); null_alt = np.full((reps, S), np.nan)
    counts = {k: dict(n=0, n_ok=0, as_dbl=0, as_sng=0, wrong=0, amb=0) for k in ("SNG", "DBL")}
    kernel_ms = 0.0
    eng = engine.Engine(len(sample_ids), alphas, device=device, mode=mode)
    eng2 = engine.Engine(len(sample_ids), alphas, device=device, mode=mode)
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        eng2.set_genotypes(g)
        a = None
        if rho is not None:
            a = amb_mod._ambient_builder(ambient, eng, g, lambda: refine.assignments_from_best(best, sample_ids, barcodes)) if isinstance(ambient, str) else ambient
        r_fit = eng.fit_profile(hyp, alpha, rho, a, max_reads)
        r_site = eng.site_fit(hyp, alpha, rho, a, max_reads)
        z_obs = fit.z_scores(r_fit["obs"], r_fit["mean"], r_fit["var"])
        zs_obs = fit.z_scores(r_site["obs"], r_site["mean"], r_site["var"])
        za_obs = fit.z_scores(r_site["exc"], np.zeros(S), r_site["vexc"])
        info = None
        with open(out_prefix + ".null.tsv", "w") as f:
            f.write(NULL_HEADER)
            for r in range(reps):
                info = eng.redraw(hyp, alpha, rho, a, seed=seed, geno_seed=geno_seed, genotype_draw=genotype_draw, index_base=r * B)
                kernel_ms += info["kernel_ms"]
                st = eng.redrawn_pileup()
                st.rd_totl, st.rd_pass, st.rd_uniq = src.rd_totl, src.rd_pass, src.rd_uniq
                engine.demuxlet_run(st, g, sample_ids, alphas, null_prefix, barcodes=barcodes, device=device, mode=mode, **demuxlet_run_kwargs)
                calls = amb_mod.read_best_rows(null_prefix + ".best", sample_ids, barcodes)
                eng2.set_pileup_struct(st, keep=pl)
                nf = eng2.fit_profile(hyp, alpha, rho, a, max_reads)
                ns = eng2.site_fit(hyp, alpha, rho, a, max_reads)
                null_fit[r] = fit.z_scores(nf["obs"], nf["mean"], nf["var"])
                null_site[r] = fit.z_scores(ns["obs"], ns["mean"], ns["var"])
                null_alt[r] = fit.z_scores(ns["exc"], np.zeros(S), ns["vexc"])
                add_counts(counts, summary_counts(hyp, calls.best, calls.sng1, calls.dbl1, calls.dbl2))
                for k in np.flatnonzero(used):
                    ok = truth_ok(int(hyp[k, 0]), int(hyp[k, 1]), calls.best[k], int(calls.sng1[k]), int(calls.dbl1[k]), int(calls.dbl2[k]))
                    f.write(f"{r}\t{barcodes[k]}\t{fit.hypothesis_label(hyp[k, 0], hyp[k, 1], alpha[k], sample_ids)}\t"
                            f"{calls.best[k] if calls.best[k] else 'NA'}\t{int(ok)}\t{fit._num(null_fit[r, k], '.4f')}\n")
    finally:
        eng2.close()
        eng.close()
    null_fit[:, ~used] = np.nan
    num = fit._num
    pe_fit = p_emp(z_obs, null_fit)
    m_fit, s_fit = null_moments(null_fit)
    with open(out_prefix + ".null_fit.tsv", "w") as f:
        f.write(NULL_FIT_HEADER)
        for k in sorted(np.flatnonzero(used), key=lambda k: barcodes[k].encode()):
            f.write(f"{barcodes[k]}\t{fit.hypothesis_label(hyp[k, 0], hyp[k, 1], alpha[k], sample_ids)}\t{num(z_obs[k], '.4f')}\t"
                    f"{num(m_fit[k], '.4f')}\t{num(s_fit[k], '.4f')}\t{num(pe_fit[k], '.6g')}\n")
    pe_site, pe_alt = p_emp(zs_obs, null_site), p_emp(za_obs, null_alt)
    m_site, s_site = null_moments(null_site)
    m_alt, s_alt = null_moments(null_alt)
    with open(out_prefix + ".null_sites.tsv", "w") as f:
        f.write(NULL_SITES_HEADER)
        for i in range(S):
            f.write(f"{i}\t{int(r_site['n_cell'][i])}\t{num(zs_obs[i], '.4f')}\t{num(m_site[i], '.4f')}\t{num(s_site[i], '.4f')}\t{num(pe_site[i], '.6g')}\t"
                    f"{num(za_obs[i], '.4f')}\t{num(m_alt[i], '.4f')}\t{num(s_alt[i], '.4f')}\t{num(pe_alt[i], '.6g')}\n")
    pooled_fit = pooled_null(null_fit[:, used], fpr)
    pooled_sites = pooled_null(null_site[:, np.asarray(r_site["n_cell"]) >= min_cells], fpr)
    write_summary_tsv(out_prefix + ".null_summary.tsv", counts, pooled_fit, pooled_sites, fpr)
    return dict(rows=rows, hyp=hyp, alpha=alpha, used=used, z_obs=z_obs, z_site_obs=zs_obs, z_alt_obs=za_obs, null_fit=null_fit,
                null_site=null_site, null_alt=null_alt, p_emp=pe_fit, p_emp_site=pe_site, p_emp_alt=pe_alt, counts=counts,
                pooled_fit=pooled_fit, pooled_sites=pooled_sites, kernel_ms=kernel_ms, info=info, ambient=a, best=best)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.redraw",
                                 description="model-drawn null pools: the calls' error rate and the fit statistics' null law at this pool's depth")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.null.best, .null.tsv, .null_fit.tsv, .null_sites.tsv, .null_summary.tsv")
    ap.add_argument("--best", help="a .best of this pileup: its calls are the hypotheses (default: run the demultiplexing pass first)")
    ap.add_argument("--reps", type=int, default=20, help="null pools to draw (default 20)")
    ap.add_argument("--genotype-draw", choices=DRAWS, default="donor", help="one genotype per donor and SNP (default), or one per pair")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--geno-seed", type=int, default=0)
    ap.add_argument("--max-reads", type=int, default=4, help=f"reads of a pair that enter the fit statistics, 1..{fit.MAX_READS} (default 4)")
    ap.add_argument("--min-cells", type=int, default=10, help="SNPs with fewer cells stay out of the pooled site quantile (default 10)")
    ap.add_argument("--fpr", type=float, default=0.001, help="the pooled null Z's quantile to report (default 0.001)")
    ap.add_argument("--singlets-only", action="store_true", help="leave the doublet calls out: their barcodes are copied unchanged")
    ap.add_argument("--ambient-tsv", help="<x>.ambient.tsv of an ambient.py run: its RHO per barcode is the soup fraction of the hypothesis")
    ap.add_argument("--ambient", choices=("reads", "genotypes", "census"), default=None,
                    help="soup ALT frequency, as for ambient.py (default reads); needs --ambient-tsv")
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.0, 0.5], help="doublet grid of the demultiplexing passes (default 0 0.5)")
    ap.add_argument("--fast", action="store_true", help="DMX_MODE_FAST for the demultiplexing passes")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    if a.ambient is not None and a.ambient_tsv is None:
        ap.error("--ambient needs --ambient-tsv")
    if a.ambient is None:
        a.ambient = "reads"
    try:
        check_args(a.reps, a.fpr, a.min_cells, a.max_reads, a.genotype_draw, a.seed, a.geno_seed)
    except ValueError as ex:
        ap.error(str(ex))
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    d = refine.read_pileup_txt(a.pileup)
    rho = fit.read_rho_tsv(a.ambient_tsv, d.barcodes) if a.ambient_tsv else None
    r = redraw_run(d.pileup, d.g, d.sample_ids, a.out, d.barcodes, best=a.best, reps=a.reps, genotype_draw=a.genotype_draw, seed=a.seed,
                   geno_seed=a.geno_seed, max_reads=a.max_reads, min_cells=a.min_cells, fpr=a.fpr, singlets_only=a.singlets_only, rho=rho,
                   ambient=a.ambient, alphas=a.alpha, device=a.gpu, mode=capi.DMX_MODE_FAST if a.fast else capi.DMX_MODE_STRICT)
    for kind in ("SNG", "DBL"):
        c = r["counts"][kind]
        print(f"{kind}: {c['n_ok']}/{c['n']} right ({c['as_dbl'] + c['as_sng']} the other kind, {c['wrong']} wrong donor, {c['amb']} AMB)", file=sys.stderr)
    for name, p in (("barcodes", r["pooled_fit"]), ("sites", r["pooled_sites"])):
        print(f"null Z of the {name}: n {p['n']}, mean {p['mean']:.4f}, sd {p['sd']:.4f}, {a.fpr:g} quantile {p['quantile']:.3f}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
