"""Donor shares of a read pool: which donors, in what proportions, make up a group of barcodes' reads.

Every stored read of a group is taken as an independent draw from a mixture of the V donors (the model ambient.py uses for soup): at SNP i
a read is ALT with probability A_i(w) = sum over v of w_v d_iv, d_iv the expected ALT dosage of donor v from the genotype matrix.  The
engine finds the maximum-likelihood shares by an EM whose iteration is one pass over the pileup (Engine.census, dmx_engine_census;
DESIGN.md section 22), accelerated by SQUAREM and stopped by the duality gap, an upper bound of the log-likelihood still to be gained.
Uses: the make-up of the soup (a group of empty droplets), the donors' cell or RNA contributions (all barcodes pooled), and whether a
donor of the VCF is in the pool at all (a share of 0).

    python -m demuxlet_amd.census --pileup <x>.pileup.txt --out <prefix> [--groups FILE | --max-reads N] [--tol T] [--max-steps M]
        [--no-accel] [--se] [--presence] [--gpu G]

reads the dump that `demuxlet --pileup-only` writes.  By default every barcode goes into one group POOL; --groups names a
BARCODE<TAB>GROUP file (barcodes not listed are left out); --max-reads N makes two groups, EMPTY (barcodes with at most N unique reads)
and CELLS.  It writes

  <prefix>.census.tsv          GROUP SM_ID SHARE READS — one row per group and donor; READS = SHARE x the group's counted reads
  <prefix>.census_groups.tsv   GROUP N.BARCODE N.SNP N.READ LLK GAP STEPS CONVERGED — N.SNP counts the (barcode, SNP) pairs that contributed
  <prefix>.census_profile.tsv  SNP GROUP A — the implied ALT frequency sum_v w_v d_iv of every SNP (NA where a donor's genotype row is
                               all zero: such SNPs are left out of the census)

Uncertainty.  --se makes one Engine.census_fisher call at the fitted shares: the observed information H of
every group and the per-barcode scores.  From them `covariance` forms two standard errors per share: the model-based one (inverse
information on the simplex), right when reads are independent draws (soup, empty droplets), and the barcode-robust sandwich, which lets
all reads of a barcode hang together and is the only honest one for groups of cells.  It writes

  <prefix>.census_se.tsv       GROUP SM_ID SHARE SE SE.ROBUST LO HI AT.BOUND — LO / HI = SHARE -/+ 1.96 SE.ROBUST clipped to [0, 1]; a donor
                               with SHARE x N.READ <= 1 is at the bound: SE 0, AT.BOUND 1; NA where H is singular on the free donors
                               (related or identical donors) or, for SE.ROBUST, the group has fewer than 2 |free donors| barcodes
  <prefix>.census_cov.tsv      GROUP SM_ID1 SM_ID2 COV COV.ROBUST — free donors only, SM_ID1 before or equal to SM_ID2 in VCF order

--presence tests every donor of every group: a refit from the fitted shares with that donor held at 0 (the donors at the bound stay
at 0, the others are renormalised; the stopping rule is the duality gap on the support of the start), LLR = max(LLK.FULL - LLK.WITHOUT, 0) and P = erfc(sqrt(LLR)) / 2, the
tail of the half-and-half mixture of chi-square 0 and chi-square 1 that a parameter on the boundary calls for.  A donor at the bound gets
LLR 0 and P 1 without a refit.  The likelihood ratio is the independent-reads model's: for groups of cells, where reads of a barcode
hang together, it is anti-conservative, and SHARE / SE.ROBUST of the --se table is the safer reading.  It writes

  <prefix>.census_presence.tsv GROUP SM_ID SHARE LLK.FULL LLK.WITHOUT LLR P STEPS CONVERGED

Both intervals and the test rest on a normal / chi-square approximation that is poor for a share near 0 or 1.  Without the two flags
the three files above keep their bytes."""
from __future__ import annotations

import argparse
import math
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import engine, refine

CENSUS_HEADER = "GROUP\tSM_ID\tSHARE\tREADS\n"
GROUPS_HEADER = "GROUP\tN.BARCODE\tN.SNP\tN.READ\tLLK\tGAP\tSTEPS\tCONVERGED\n"
PROFILE_HEADER = "SNP\tGROUP\tA\n"
SE_HEADER = "GROUP\tSM_ID\tSHARE\tSE\tSE.ROBUST\tLO\tHI\tAT.BOUND\n"
COV_HEADER = "GROUP\tSM_ID1\tSM_ID2\tCOV\tCOV.ROBUST\n"
PRESENCE_HEADER = "GROUP\tSM_ID\tSHARE\tLLK.FULL\tLLK.WITHOUT\tLLR\tP\tSTEPS\tCONVERGED\n"
MAX_GROUPS = 1024           # dmx_engine_census's most groups
MAX_SE_SAMPLES = 128        # dmx_engine_census_fisher's most donors


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


def sum_zero_basis(f: int) -> np.ndarray:
    """Q[f][f - 1]: orthonormal columns that each sum to zero (Helmert's), a basis of the directions that keep shares summing to 1."""
    Q = np.zeros((f, max(f - 1, 0)))
    for k in range(1, f):
        Q[:k, k - 1] = 1.0 / math.sqrt(k * (k + 1.0))
        Q[k, k - 1] = -k / math.sqrt(k * (k + 1.0))
    return Q


def covariance(H, w, n_read, score, n_b, min_reads: float = 1.0) -> dict:
    """Covariances of one group's fitted shares w[V] from its observed information H[V][V] (Engine.census_fisher at w), its counted
    reads N and its barcodes' score rows score[Bg][V] with their counted reads n_b[Bg].

    A donor with w_v N <= min_reads is AT THE BOUND: SE 0, left out of the free set F.  With Q an orthonormal basis of the sum-zero
    vectors of R^|F| and G1 = Q' H_FF Q:
      model   C   = Q G1^-1 Q'                                  (inverse information on the simplex: reads independent);
      robust  C_r = Bg / (Bg - 1) Q G1^-1 (Q' J Q) G1^-1 Q',    J = sum_b s_b s_b', s_b = score_b[F] - n_b 1 (the barcode's score of
                    the log-likelihood on the simplex), the sum over the Bg barcodes with a counted read.
    G1 singular (condition number above 1e12, or not finite): both are NaN on F.  Bg < 2 |F|: the robust one is NaN.
    Cross-check at a converged fit (acc_v = N on F, hence H_FF w_F = N 1): C = H_FF^-1 - w_F w_F' / N.
    Returns dict(se[V], se_robust[V], cov[V][V], cov_robust[V][V], at_bound[V] bool, free[|F|] indices, n_barcode=Bg)."""
    H = np.asarray(H, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    V = w.shape[0]
    if H.shape != (V, V):
        raise ValueError(f"H {H.shape} for {V} shares")
    score = np.asarray(score, dtype=np.float64).reshape(-1, V)
    n_b = np.asarray(n_b, dtype=np.float64)
    if n_b.shape != (score.shape[0],):
        raise ValueError(f"n_b {n_b.shape} for {score.shape[0]} score rows")
    N = float(n_read)
    at_bound = ~(w * N > min_reads)
    F = np.flatnonzero(~at_bound)
    f = len(F)
    cov = np.zeros((V, V)); cov_r = np.zeros((V, V))
    used = n_b > 0
    Bg = int(used.sum())
    if f >= 2:
        Q = sum_zero_basis(f)
        G1 = Q.T @ H[np.ix_(F, F)] @ Q
        ok = bool(np.isfinite(G1).all())
        if ok:
            sv = np.linalg.svd(G1, compute_uv=False)
            ok = bool(sv[-1] > 0.0 and sv[0] / sv[-1] <= 1e12)
        if ok:
            Gi = np.linalg.inv(G1)
            Gi = 0.5 * (Gi + Gi.T)
            cov[np.ix_(F, F)] = Q @ Gi @ Q.T
            if Bg >= 2 * f:
                s = (score[used][:, F] - n_b[used][:, None]) @ Q
                M = Gi @ (s.T @ s) @ Gi
                cov_r[np.ix_(F, F)] = (Bg / (Bg - 1.0)) * (Q @ M @ Q.T)
            else:
                cov_r[np.ix_(F, F)] = np.nan
        else:
            cov[np.ix_(F, F)] = np.nan
            cov_r[np.ix_(F, F)] = np.nan
    with np.errstate(invalid="ignore"):
        se = np.sqrt(np.maximum(np.diag(cov), 0.0))
        se_r = np.sqrt(np.maximum(np.diag(cov_r), 0.0))
    se = np.where(np.isnan(np.diag(cov)), np.nan, se)
    se_r = np.where(np.isnan(np.diag(cov_r)), np.nan, se_r)
    return dict(se=se, se_robust=se_r, cov=cov, cov_robust=cov_r, at_bound=at_bound, free=F, n_barcode=Bg)


def _num(x: float, fmt: str) -> str:
    return "NA" if not math.isfinite(x) else format(x, fmt)


def write_se_tsv(path: str, names: Sequence[str], sample_ids: Sequence[str], w: np.ndarray, covs: Sequence[dict]) -> None:
    with open(path, "w") as f:
        f.write(SE_HEADER)
        for k, name in enumerate(names):
            c = covs[k]
            for v, s in enumerate(sample_ids):
                sr = float(c["se_robust"][v])
                lo = min(max(w[k, v] - 1.96 * sr, 0.0), 1.0) if math.isfinite(sr) else math.nan
                hi = min(max(w[k, v] + 1.96 * sr, 0.0), 1.0) if math.isfinite(sr) else math.nan
                f.write(f"{name}\t{s}\t{w[k, v]:.6f}\t{_num(float(c['se'][v]), '.6f')}\t{_num(sr, '.6f')}\t{_num(lo, '.6f')}\t{_num(hi, '.6f')}\t"
                        f"{int(c['at_bound'][v])}\n")


def write_cov_tsv(path: str, names: Sequence[str], sample_ids: Sequence[str], covs: Sequence[dict]) -> None:
    with open(path, "w") as f:
        f.write(COV_HEADER)
        for k, name in enumerate(names):
            c = covs[k]
            for a in c["free"]:
                for b in c["free"]:
                    if a <= b:
                        f.write(f"{name}\t{sample_ids[a]}\t{sample_ids[b]}\t{_num(float(c['cov'][a, b]), '.6e')}\t"
                                f"{_num(float(c['cov_robust'][a, b]), '.6e')}\n")


def write_presence_tsv(path: str, names: Sequence[str], sample_ids: Sequence[str], w: np.ndarray, ll_full, pres: dict) -> None:
    with open(path, "w") as f:
        f.write(PRESENCE_HEADER)
        for k, name in enumerate(names):
            for v, s in enumerate(sample_ids):
                f.write(f"{name}\t{s}\t{w[k, v]:.6f}\t{ll_full[k]:.5f}\t{pres['ll_without'][k, v]:.5f}\t{pres['llr'][k, v]:.5f}\t"
                        f"{pres['p'][k, v]:.4g}\t{int(pres['n_steps'][k, v])}\t{int(pres['converged'][k, v])}\n")


def presence_p(llr):
    """P of the boundary likelihood-ratio test: half chi-square 0, half chi-square 1 on 2 LLR, i.e. erfc(sqrt(LLR)) / 2."""
    return np.array([0.5 * math.erfc(math.sqrt(max(float(x), 0.0))) for x in np.ravel(llr)]).reshape(np.shape(llr))


def presence_start(w: np.ndarray, v: int, hold=None) -> np.ndarray:
    """w[G][V] with donor v zeroed, the entries of the mask hold[G][V] zeroed as well, and every row renormalised (a row with nothing
    left becomes uniform over the donors other than v)."""
    x = np.array(w, dtype=np.float64)
    if hold is not None:
        x[np.asarray(hold, dtype=bool)] = 0.0
    x[:, v] = 0.0
    s = x.sum(axis=1)
    lone = ~(s > 0.0)
    if lone.any():
        x[lone] = 1.0
        x[lone, v] = 0.0
        s = x.sum(axis=1)
    x = x / s[:, None]
    return x / x.sum(axis=1)[:, None]           # (a second division brings a row sum that is an ulp off back within 1e-12)


def presence_test(census_fn, w: np.ndarray, ll_full, n_read, min_reads: float = 1.0) -> dict:
    """For every donor v: census_fn(w0) -> dict(w, ll, n_steps, converged) refits all groups from w0 = presence_start(w, v, bound) with
    the gap on the start's support; LLR[g][v] = max(ll_full[g] - ll[g], 0).  A donor at the bound in a group (w N <= min_reads) gets
    LLR 0, P 1, STEPS 0 there; a donor at the bound in every group is not refitted at all.  The donors at the bound stay at 0 in every
    refit of their group: a share of 1e-10 left in the support creeps up by a factor acc_v / N = 1 + 1e-5 per pass once another donor
    is taken out and keeps the gap above tol for thousands of passes; LLK.WITHOUT is then the likelihood of the free donors without v,
    below the one with the bound donors let in by at most their part of the full fit's gap.
    The refit for donor v runs over every group, those where v is at the bound included, and their results are not used: the engine's
    call has no way to leave a group out.  Such a group starts from its fitted shares, which stop at once when the full fit converged;
    where it did not, the group spends up to max_steps further passes for nothing.
    Returns dict(ll_without, llr, p, n_steps, converged), each [G][V]."""
    w = np.asarray(w, dtype=np.float64)
    G, V = w.shape
    if V < 2:
        raise ValueError("presence: at least two donors needed")
    ll_full = np.asarray(ll_full, dtype=np.float64)
    bound = ~(w * np.asarray(n_read, dtype=np.float64)[:, None] > min_reads)
    ll_wo = np.repeat(ll_full[:, None], V, axis=1)
    steps = np.zeros((G, V), dtype=np.int64); conv = np.ones((G, V), dtype=np.int64)
    for v in range(V):
        if bound[:, v].all():
            continue
        r = census_fn(presence_start(w, v, bound))
        free = ~bound[:, v]
        ll_wo[free, v] = np.asarray(r["ll"])[free]
        steps[free, v] = np.asarray(r["n_steps"])[free]
        conv[free, v] = np.asarray(r["converged"])[free]
    llr = np.maximum(ll_full[:, None] - ll_wo, 0.0)
    llr[bound] = 0.0
    p = presence_p(llr)
    p[bound] = 1.0
    return dict(ll_without=ll_wo, llr=llr, p=p, n_steps=steps, converged=conv)


def census_run(store_or_pileup, g: np.ndarray, sample_ids: Sequence[str], out_prefix: Optional[str], groups=None, max_reads: Optional[int] = None,
               tol: float = 1e-4, max_steps: int = 2000, accelerate: bool = True, gpu: int = 0, barcodes: Optional[Sequence[str]] = None,
               snps=None, se: bool = False, presence: bool = False) -> dict:
    """The census of `store_or_pileup` (a Store, or a HostPileup) against genotype matrix g.  `groups` is None (one group POOL of every
    barcode), a BARCODE<TAB>GROUP path (needs the barcodes: a Store's own, or barcodes=), or a pair (group[B] int array, names);
    max_reads=N instead makes the groups EMPTY / CELLS.  Writes the three files unless out_prefix is None; returns a dict with the
    engine's results (w, ll, gap, n_steps, converged, n_read, n_pair), group, names, n_barcode, profile[G][S] and info.
    se=True adds one Engine.census_fisher call at the fitted shares, `covariance` per group (key "cov": a list of its dicts; "fisher":
    the call's results) and the files .census_se.tsv / .census_cov.tsv; presence=True adds the donor presence tests (key "presence") and
    .census_presence.tsv."""
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
    if se and len(sample_ids) > MAX_SE_SAMPLES:
        raise ValueError(f"census_run: se needs at most {MAX_SE_SAMPLES} samples, not {len(sample_ids)}")
    if presence and len(sample_ids) < 2:
        raise ValueError("census_run: presence needs at least two samples")
    extra = {}
    eng = engine.Engine(len(sample_ids), device=gpu)
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        r = eng.census(group, n_groups=len(names), tol=tol, max_steps=max_steps, accelerate=accelerate)
        info = eng.census_info()
        if se:
            fi = eng.census_fisher(group, r["w"], n_groups=len(names))
            extra["fisher"] = fi
            extra["cov"] = [covariance(fi["H"][k], r["w"][k], r["n_read"][k], fi["score"][group == k], fi["n_read_b"][group == k])
                            for k in range(len(names))]
        if presence:
            extra["presence"] = presence_test(
                lambda w0: eng.census(group, n_groups=len(names), w0=w0, tol=tol, max_steps=max_steps, accelerate=accelerate,
                                      gap_on_support=True), r["w"], r["ll"], r["n_read"])
    finally:
        eng.close()
    profile = np.stack([ambient_profile(r["w"][k], g) for k in range(len(names))])
    n_bar = np.bincount(group[group >= 0], minlength=len(names))
    if out_prefix is not None:
        write_census_tsv(out_prefix + ".census.tsv", names, sample_ids, r["w"], r["n_read"])
        write_groups_tsv(out_prefix + ".census_groups.tsv", names, n_bar, r)
        write_profile_tsv(out_prefix + ".census_profile.tsv", names, profile, snps)
        if se:
            write_se_tsv(out_prefix + ".census_se.tsv", names, sample_ids, r["w"], extra["cov"])
            write_cov_tsv(out_prefix + ".census_cov.tsv", names, sample_ids, extra["cov"])
        if presence:
            write_presence_tsv(out_prefix + ".census_presence.tsv", names, sample_ids, r["w"], r["ll"], extra["presence"])
    return dict(r, group=group, names=names, n_barcode=n_bar, profile=profile, info=info, **extra)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.census", description="donor shares of a pool of reads")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.census.tsv, <out>.census_groups.tsv, <out>.census_profile.tsv")
    ap.add_argument("--groups", help="BARCODE<TAB>GROUP file (default: one group POOL of every barcode)")
    ap.add_argument("--max-reads", type=int, help="two groups: EMPTY = barcodes with at most N unique reads, CELLS = the others")
    ap.add_argument("--tol", type=float, default=1e-4, help="stop a group at duality gap <= this, in log-likelihood units (default 1e-4)")
    ap.add_argument("--max-steps", type=int, default=2000, help="passes per group at most (default 2000)")
    ap.add_argument("--no-accel", action="store_true", help="plain EM instead of SQUAREM")
    ap.add_argument("--se", action="store_true", help="standard errors of the shares, model-based and barcode-robust: <out>.census_se.tsv, "
                    "<out>.census_cov.tsv (at most 128 samples)")
    ap.add_argument("--presence", action="store_true", help="likelihood-ratio test of every donor's presence: <out>.census_presence.tsv")
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
                   accelerate=not a.no_accel, gpu=a.gpu, barcodes=d.barcodes, snps=d.snps, se=a.se, presence=a.presence)
    for k, name in enumerate(r["names"]):
        top = int(np.argmax(r["w"][k]))
        print(f"{name}: {int(r['n_read'][k])} reads, {int(r['n_steps'][k])} steps, gap {r['gap'][k]:.3g}; largest share "
              f"{d.sample_ids[top]} {r['w'][k, top]:.4f}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
