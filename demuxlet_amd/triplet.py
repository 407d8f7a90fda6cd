"""Triplet calls: flag the barcodes that the pair model does not explain.

The plain pass scores singlets and doublets only, so a droplet with three donors gets a confident-looking `DBL-a-b` for two of them.
This pass takes each barcode's best pairs from a `.best` (slot 0 = (DBL.1ST, DBL.2ND), slot 1 = (SNG.1ST, SNG.2ND) when that is a different
unordered pair; ambient.candidates_from_best) and scores every sample of the pool as a third donor over a small grid of read shares
(w1, w2, w3) (Engine.triplet_profile / dmx_engine_triplet).  The singlet and doublet baselines come from the ambient kernels at rho = 0
(Engine.ambient_profile / ambient_doublet_profile), which are on the same scale: no per-read renormalisation, no floor.

    LLK.TRP = max over used slots, share triples and third donors c outside the slot's pair   (lowest index on ties: slot, share, c)
    CALL    = TRP-a-b-c-w1/w2/w3  if LLK.TRP > max(LLK.DBL, LLK.SNG1) + 2,  else ambient.decide's SNG- / DBL- / AMB- (section 18)

A comparison that ties at the margin is not won.  One base pair plus a third donor is searched, not all V^3 triples; there is no soup
term; the shares are a grid, not a fit; more than three donors are not modelled.

    python -m demuxlet_amd.triplet --pileup <x>.pileup.txt --out <prefix> [--best <x>.best] [--shares w1,w2,w3 ...] [--alpha A ...]
                                   [--dbl-alpha A ...] [--fast] [--gpu G]

writes <prefix>.triplet.tsv (and, without --best, the plain <prefix>.best/.single/.sing2 first)."""
import argparse
import sys
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import ambient, capi, engine, refine

MAX_SHARES = 8              # dmx_engine_triplet's longest share grid
SHARE_SUM_TOL = 1e-12
CALL_TRP = 3                # beside ambient.CALL_SNG / CALL_DBL / CALL_AMB
TRIPLET_HEADER = ("BARCODE\tBEST\tCALL\tSNG.1ST\tLLK.SNG1\tSNG.2ND\tLLK.SNG2\tDBL.1ST\tDBL.2ND\tALPHA\tLLK.DBL\tTRP.1ST\tTRP.2ND\tTRP.3RD\t"
                  "SHARES\tLLK.TRP\tLLR\tN.SNP\tN.READ\n")


def default_shares() -> np.ndarray:
    """Even thirds, and each donor in turn with half of the reads."""
    return np.array([[1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0], [0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]])


def check_shares(shares, allow_zero: bool = False) -> np.ndarray:
    """dmx_engine_triplet's rules: 1 to 8 rows (w1, w2, w3) in [0, 1], |w1 + w2 + w3 - 1| <= 1e-12, pairwise different.  Unless
    allow_zero, every share must also be > 0: with a zero share the model is the doublet one."""
    sh = np.ascontiguousarray(shares, dtype=np.float64)
    if sh.ndim != 2 or sh.shape[1] != 3 or not 1 <= sh.shape[0] <= MAX_SHARES:
        raise ValueError(f"shares: 1 to {MAX_SHARES} rows of three values, got {sh.shape}")
    if not np.all((sh >= 0.0) & (sh <= 1.0)):
        raise ValueError("shares: every value must be in [0, 1]")
    if not allow_zero and not np.all(sh > 0.0):
        raise ValueError("shares: every value must be > 0 (with a zero share the triplet model is the doublet one)")
    if not np.all(np.abs(sh[:, 0] + sh[:, 1] + sh[:, 2] - 1.0) <= SHARE_SUM_TOL):
        raise ValueError("shares: every row must sum to 1")
    for t in range(len(sh)):
        for u in range(t):
            if np.array_equal(sh[t], sh[u]):
                raise ValueError(f"shares: row {t} repeats row {u}")
    return sh


def decide(llk_sng1, llk_sng2, llk_dbl, llk_trp) -> np.ndarray:
    """CALL_TRP if LLK.TRP > max(LLK.DBL, LLK.SNG1) + 2; otherwise ambient.decide.  A tie at the margin is not won."""
    s1, d, t = (np.asarray(x, dtype=np.float64) for x in (llk_sng1, llk_dbl, llk_trp))
    return np.where(t > np.maximum(d, s1) + ambient.CALL_MARGIN, CALL_TRP, ambient.decide(llk_sng1, llk_sng2, llk_dbl)).astype(np.int32)


@dataclass
class Calls:
    """Triplet-aware calls per cell id (meaningless where the `.best` has no row)."""
    call: np.ndarray         # ambient.CALL_SNG / CALL_DBL / CALL_AMB or CALL_TRP
    llk_sng1: np.ndarray
    llk_sng2: np.ndarray
    dbl1: np.ndarray         # the doublet candidate of the highest LL (-1: the barcode had no candidate pair)
    dbl2: np.ndarray
    alpha: np.ndarray
    llk_dbl: np.ndarray
    trp1: np.ndarray         # the base pair and third donor of the highest LL (-1: none)
    trp2: np.ndarray
    trp3: np.ndarray
    share: np.ndarray        # index into the share grid
    llk_trp: np.ndarray
    llr: np.ndarray          # LLK.TRP - max(LLK.DBL, LLK.SNG1)


def make_calls(rows: ambient.BestRows, cand: np.ndarray, ll_sng1, ll_sng2, ll_dbl, dbl_alphas, ll_trp) -> Calls:
    """Maxima of the singlet values [B], of the doublet profile [B][C][A] and of the triplet profile [B][C][T][V] (lowest index on ties:
    slot, alpha / slot, share, c; unused slots, an absent SNG.2ND and a third donor inside the slot's pair count as -inf), then decide()."""
    al = np.asarray(dbl_alphas, dtype=np.float64)
    B = len(rows.sng1)
    rb = np.arange(B)
    used = cand[:, :, 0] >= 0
    l1 = np.asarray(ll_sng1, dtype=np.float64)
    l2 = np.where(rows.sng2 >= 0, np.asarray(ll_sng2, dtype=np.float64), -np.inf)
    Cn, A = ll_dbl.shape[1:]
    x = np.where(used[:, :, None], ll_dbl, -np.inf).reshape(B, Cn * A)
    td = np.argmax(x, axis=1) if B else np.zeros(0, dtype=np.int64)
    ld = x[rb, td]
    cd, nd = td // A, td % A
    none = ~used.any(axis=1)
    Ct, T, V = ll_trp.shape[1:]
    cols = np.arange(V)[None, None, :]
    third = used[:, :, None] & (cols != cand[:, :, 0:1]) & (cols != cand[:, :, 1:2])           # [B][C][V]
    y = np.where(third[:, :, None, :], ll_trp, -np.inf).reshape(B, Ct * T * V)
    tt = np.argmax(y, axis=1) if B else np.zeros(0, dtype=np.int64)
    lt = y[rb, tt] if B else np.zeros(0)
    ct, st, vt = tt // (T * V), (tt // V) % T, tt % V
    no_trp = ~third.any(axis=(1, 2))
    lt = np.where(no_trp, -np.inf, lt)
    with np.errstate(invalid="ignore"):
        llr = lt - np.maximum(ld, l1)
    return Calls(decide(l1, l2, ld, lt), l1, l2, np.where(none, -1, cand[rb, cd, 0]), np.where(none, -1, cand[rb, cd, 1]), al[nd], ld,
                 np.where(no_trp, -1, cand[rb, ct, 0]), np.where(no_trp, -1, cand[rb, ct, 1]), np.where(no_trp, -1, vt), st, lt, llr)


def shares_string(w) -> str:
    return "/".join(f"{x:.3f}" for x in w)


def call_string(k: int, rows: ambient.BestRows, calls: Calls, sample_ids: Sequence[str], shares) -> str:
    """TRP-a-b-c-w1/w2/w3, or section 18's SNG-x / DBL-x-y-alpha / AMB-x-y-j/k."""
    name = lambda j: sample_ids[int(j)] if j >= 0 else "."
    if calls.call[k] == CALL_TRP:
        return f"TRP-{name(calls.trp1[k])}-{name(calls.trp2[k])}-{name(calls.trp3[k])}-{shares_string(shares[calls.share[k]])}"
    return ambient.call_string(k, rows, calls, sample_ids)


def write_triplet_tsv(path: str, barcodes: Sequence[str], sample_ids: Sequence[str], rows: ambient.BestRows, calls: Calls, shares, n_snp,
                      n_read) -> None:
    """One row per barcode of the `.best`, in ascending byte-wise barcode order (the writers' order); `.` where there is no candidate."""
    name = lambda j: sample_ids[int(j)] if j >= 0 else "."
    num = lambda x: f"{x:.5f}" if np.isfinite(x) else "."
    order = sorted(np.flatnonzero(rows.has_row), key=lambda k: barcodes[k].encode())
    with open(path, "w") as f:
        f.write(TRIPLET_HEADER)
        for k in order:
            c = calls
            f.write(f"{barcodes[k]}\t{rows.best[k]}\t{call_string(k, rows, c, sample_ids, shares)}\t{name(rows.sng1[k])}\t{num(c.llk_sng1[k])}\t"
                    f"{name(rows.sng2[k])}\t{num(c.llk_sng2[k])}\t{name(c.dbl1[k])}\t{name(c.dbl2[k])}\t"
                    f"{f'{c.alpha[k]:.3f}' if c.dbl1[k] >= 0 else '.'}\t{num(c.llk_dbl[k])}\t{name(c.trp1[k])}\t{name(c.trp2[k])}\t{name(c.trp3[k])}\t"
                    f"{shares_string(shares[c.share[k]]) if c.trp1[k] >= 0 else '.'}\t{num(c.llk_trp[k])}\t{num(c.llr[k])}\t{int(n_snp[k])}\t"
                    f"{int(n_read[k])}\n")


def triplet_run(store_or_pileup, g: np.ndarray, sample_ids: Sequence[str], out_prefix: str, best: Optional[str] = None, shares=None,
                alphas: Sequence[float] = (0.0, 0.5), dbl_alphas=None, barcodes: Optional[Sequence[str]] = None, device: int = 0,
                mode: int = capi.DMX_MODE_STRICT, **demuxlet_run_kwargs):
    """Call every barcode of `best` (a `.best` path) again with a triplet hypothesis beside the singlet and doublet ones.  Without `best`,
    the unchanged demuxlet_run writes <out_prefix>.best/.single/.sing2 first.  `shares` defaults to default_shares(), `dbl_alphas` to the
    values of `alphas` above 0.  `store_or_pileup` is a Store, or a HostPileup with barcodes=... as for demuxlet_run.  Writes
    <out_prefix>.triplet.tsv; returns a dict with the rows, base pairs, the profiles and the calls."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    sh = default_shares() if shares is None else check_shares(shares)
    dal = ambient.dbl_alphas_from_run(alphas) if dbl_alphas is None else ambient.check_dbl_alphas(dbl_alphas)
    if isinstance(store_or_pileup, engine.HostPileup):
        pl = store_or_pileup
        if barcodes is None:
            raise ValueError("triplet_run: a HostPileup needs barcodes=")
    else:
        pl, barcodes = store_or_pileup.freeze(), store_or_pileup.barcodes()
    if g.ndim != 3 or g.shape[0] != pl.n_snps or g.shape[1] != len(sample_ids) or g.shape[2] != 3:
        raise ValueError(f"genotype matrix {g.shape} for {pl.n_snps} SNPs and {len(sample_ids)} samples")
    if best is None:
        engine.demuxlet_run(pl, g, sample_ids, alphas, out_prefix, barcodes=barcodes, device=device, mode=mode, **demuxlet_run_kwargs)
        best = out_prefix + ".best"
    rows = ambient.read_best_rows(best, sample_ids, barcodes)
    cand = ambient.candidates_from_best(rows)
    zeros, rho0 = np.zeros(pl.n_snps), np.zeros(1)
    eng = engine.Engine(len(sample_ids), alphas, device=device, mode=mode)
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        ll1, n_snp, n_read = eng.ambient_profile(rows.sng1, zeros, rho0)
        ll2, _, _ = eng.ambient_profile(rows.sng2, zeros, rho0)
        lld, _, _ = eng.ambient_doublet_profile(cand, dal, zeros, rho0)
        llt, _, _ = eng.triplet_profile(cand, sh)
        info = eng.triplet_info()
    finally:
        eng.close()
    ll1, ll2, lld = ll1[:, 0], ll2[:, 0], lld[:, :, :, 0]
    calls = make_calls(rows, cand, ll1, ll2, lld, dal, llt)
    write_triplet_tsv(out_prefix + ".triplet.tsv", barcodes, sample_ids, rows, calls, sh, n_snp, n_read)
    return dict(rows=rows, cand=cand, shares=sh, dbl_alphas=dal, ll_sng1=ll1, ll_sng2=ll2, ll_dbl=lld, ll_trp=llt, n_snp=n_snp, n_read=n_read,
                calls=calls, info=info)


def parse_shares(text: str):
    t = text.split(",")
    if len(t) != 3:
        raise ValueError(f"--shares {text!r}: three comma-separated values w1,w2,w3")
    return [float(x) for x in t]


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.triplet", description="triplet calls: every best pair with a third donor")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.triplet.tsv (and <out>.best/... without --best)")
    ap.add_argument("--best", help="a .best of this pileup (default: run the demultiplexing pass first)")
    ap.add_argument("--shares", nargs="+", metavar="W1,W2,W3",
                    help="read shares of the base pair's two donors and the third, each > 0 and summing to 1 (default: thirds and 0.5/0.25/0.25 in turn)")
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.0, 0.5], help="doublet grid of the demultiplexing pass (default 0 0.5)")
    ap.add_argument("--dbl-alpha", type=float, nargs="+",
                    help="mixing shares of the doublet baseline, in (0, 1] (default: the --alpha values above 0)")
    ap.add_argument("--fast", action="store_true", help="DMX_MODE_FAST for the demultiplexing pass")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    try:
        a.shares = check_shares([parse_shares(s) for s in a.shares]) if a.shares is not None else default_shares()
        a.dbl_alpha = ambient.check_dbl_alphas(a.dbl_alpha) if a.dbl_alpha is not None else ambient.dbl_alphas_from_run(a.alpha)
    except ValueError as ex:
        ap.error(str(ex))
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    d = refine.read_pileup_txt(a.pileup)
    r = triplet_run(d.pileup, d.g, d.sample_ids, a.out, best=a.best, shares=a.shares, alphas=a.alpha, dbl_alphas=a.dbl_alpha,
                    barcodes=d.barcodes, device=a.gpu, mode=capi.DMX_MODE_FAST if a.fast else capi.DMX_MODE_STRICT)
    n = np.bincount(r["calls"].call[r["rows"].has_row], minlength=4)
    print(f"triplet-aware calls: {n[ambient.CALL_SNG]} SNG, {n[ambient.CALL_DBL]} DBL, {n[ambient.CALL_AMB]} AMB, {n[CALL_TRP]} TRP", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
