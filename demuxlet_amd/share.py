"""Unequal doublets: scan every partner of a barcode's best singlets and fit a continuous mixing share.

Every pass that names a doublet scores it at the shares the user lists (default 0 and 0.5).  A droplet of a large and a small cell sends
10-25 % of its reads from the minor donor; at alpha = 0.5 that fits worse than the major donor's singlet, so the plain pass prints SNG-.
This pass treats the share as a parameter, on the scale of ambient.py (no per-read renormalisation, no floor):

  1. anchors: the barcode's --anchors best singlets (Engine.get_singlet; the first maximum in ascending sample order);
  2. scan (Engine.share_scan, dmx_engine_share_scan): for every anchor and EVERY other sample v, LL, LL' and LL'' in the share of v's reads
     at alpha = 0; the score statistic z = LL'(0) / sqrt(-LL''(0)) ranks the partners.  Per barcode the --top partners of highest z are kept,
     over the anchors, only where LL'(0) > 0 and LL''(0) < 0, ties by ascending (anchor slot, v), an unordered pair once; the plain pass's
     (DBL.1ST, DBL.2ND) is always added;
  3. fit (Engine.share_fit, dmx_engine_share_fit): a safeguarded Newton iteration on [0, 1] per kept pair gives alpha_hat, LL, LL', LL''
     there and at both ends, which are the two singlets on this scale;
  4. LLK.SNG = the largest end value over the pairs, LLK.DBL = the largest LL(alpha_hat) over the pairs whose maximum is interior;
     CALL = DBL-a-b-alpha when LLK.DBL - LLK.SNG > 2 (the reference's margin), a the donor with the larger share and alpha the share of b;
     else SNG-j, j the singlet of LLK.SNG.

  <prefix>.share.tsv       BARCODE BEST CALL DONOR1 DONOR2 ALPHA SE LO HI LLK.SNG LLK.HALF LLK.HAT LLR Z.SCAN N.EVAL STATUS N.SNP N.READ — one
                           row per barcode of the `.best`, in byte-wise barcode order.  DONOR1 .. N.READ describe the barcode's best pair: the
                           interior pair of the highest LL(alpha_hat), or without one the pair that holds LLK.SNG.  SE = 1 / sqrt(-LL''(alpha_hat)),
                           LO / HI = ALPHA -+ 1.96 SE clipped to [0, 1] (a Wald interval), LLK.HALF = LL(0.5) of that pair, LLK.HAT = LL(alpha_hat);
                           NA where a value does not exist
  <prefix>.share_scan.tsv  BARCODE ANCHOR PARTNER Z LLK0 D1 D2 — the kept partners

`.best` is never changed.  Limits: two donors; with soft genotype rows LL need not be concave and the fit finds a local maximum; the
interval is Wald's; rho is taken (from --ambient-tsv), not fitted; the top partners are selected on the host, so B x T x V x 3 doubles
come back from the scan; one GPU.

    python -m demuxlet_amd.share --pileup <x>.pileup.txt --out <prefix> [--best <x>.best] [--anchors T] [--top C]
        [--ambient-tsv <x>.ambient.tsv [--ambient reads|genotypes|census]] [--tol T] [--max-iter N] [--alpha A ...] [--fast] [--gpu G]

reads the dump that `demuxlet --pileup-only` writes.  Without --best, the unchanged demultiplexing pass runs first and writes
<prefix>.best/.single/.sing2."""
from __future__ import annotations

import argparse
import math
import sys
from typing import Optional, Sequence

import numpy as np

from . import capi, engine, refine

MAX_ANCHORS = 4             # dmx_engine_share_scan's most anchor slots
MAX_CAND = 8                # dmx_engine_share_fit's most candidate slots: --top partners and the plain pass's pair
MAX_SAMPLES = 1024
CALL_MARGIN = 2.0           # the reference's margin between two log-likelihoods
SHARE_HEADER = ("BARCODE\tBEST\tCALL\tDONOR1\tDONOR2\tALPHA\tSE\tLO\tHI\tLLK.SNG\tLLK.HALF\tLLK.HAT\tLLR\tZ.SCAN\tN.EVAL\tSTATUS\t"
                "N.SNP\tN.READ\n")
SCAN_HEADER = "BARCODE\tANCHOR\tPARTNER\tZ\tLLK0\tD1\tD2\n"
STATUS_NAMES = ((capi.DMX_SHARE_INTERIOR, "INTERIOR"), (capi.DMX_SHARE_AT_0, "AT_0"), (capi.DMX_SHARE_AT_1, "AT_1"),
                (capi.DMX_SHARE_NOT_CONVERGED, "NOT_CONVERGED"), (capi.DMX_SHARE_FLAT, "FLAT"), (capi.DMX_SHARE_NONFINITE, "NONFINITE"))


def anchors_from_singlet(llks: np.ndarray, n_anchor: int) -> np.ndarray:
    """anchors[B][T]: each barcode's T best singlets, the first maximum in ascending sample order first; -1 past the pool's size."""
    llks = np.asarray(llks, dtype=np.float64)
    B, V = llks.shape
    order = np.argsort(-llks, axis=1, kind="stable")[:, :n_anchor].astype(np.int32)
    out = np.full((B, n_anchor), -1, dtype=np.int32)
    out[:, :order.shape[1]] = order
    return out


def scan_z(scan: np.ndarray) -> np.ndarray:
    """z = LL'(0) / sqrt(-LL''(0)) where LL'(0) > 0 and LL''(0) < 0, NaN elsewhere; scan[...][3] = (LL, LL', LL'')."""
    d1, d2 = scan[..., 1], scan[..., 2]
    with np.errstate(invalid="ignore"):
        ok = (d1 > 0.0) & (d2 < 0.0)
        return np.where(ok, d1 / np.sqrt(np.where(ok, -d2, 1.0)), np.nan)


def select_candidates(scan: np.ndarray, anchors: np.ndarray, top: int, dbl1=None, dbl2=None):
    """cand[B][top + 1][2] for Engine.share_fit and pick[B][top + 1][2] = the (anchor slot, partner) each slot came from (-1, -1 for the
    plain pass's pair and for unused slots).  Per barcode the `top` entries of highest z over (t, v), ties by ascending (t, v), an
    unordered pair kept once; then (dbl1[b], dbl2[b]) unless it is among them already, is not two different samples, or is absent."""
    B, T, V, _ = scan.shape
    z = scan_z(scan)
    cand = np.full((B, top + 1, 2), -1, dtype=np.int32)
    pick = np.full((B, top + 1, 2), -1, dtype=np.int32)
    for b in range(B):
        zb = z[b].reshape(-1)
        idx = np.flatnonzero(np.isfinite(zb) & np.repeat(anchors[b] >= 0, V))
        idx = idx[np.argsort(-zb[idx], kind="stable")]            # flat index = t V + v: a stable sort breaks ties by ascending (t, v)
        seen, n = set(), 0
        for k in idx:
            t, v = divmod(int(k), V)
            a = int(anchors[b, t])
            key = (min(a, v), max(a, v))
            if a == v or key in seen:
                continue
            seen.add(key)
            cand[b, n] = (a, v)
            pick[b, n] = (t, v)
            n += 1
            if n == top:
                break
        if dbl1 is not None:
            a, v = int(dbl1[b]), int(dbl2[b])
            if a >= 0 and v >= 0 and a != v and (min(a, v), max(a, v)) not in seen:
                cand[b, n] = (a, v)
    return cand, pick


def decide(fit: dict, cand: np.ndarray) -> dict:
    """The call per barcode from Engine.share_fit's arrays.  Returns llk_sng, sng (the singlet that holds it), llk_dbl, best (the slot of
    the barcode's best pair: the interior pair of the highest LL(alpha_hat), else the pair that holds llk_sng, -1 without a used slot) and
    is_dbl (llk_dbl - llk_sng > CALL_MARGIN).  The first maximum in slot order wins, LL(0) before LL(1)."""
    B, Cn = cand.shape[:2]
    used = cand[:, :, 0] >= 0
    llk_sng = np.full(B, np.nan); llk_dbl = np.full(B, np.nan)
    sng = np.full(B, -1, dtype=np.int32); best = np.full(B, -1, dtype=np.int32)
    for b in range(B):
        s_slot = d_slot = -1
        for c in range(Cn):
            if not used[b, c]:
                continue
            for end, v in ((fit["ll0"][b, c], cand[b, c, 0]), (fit["ll1"][b, c], cand[b, c, 1])):
                if np.isfinite(end) and (s_slot < 0 or end > llk_sng[b]):
                    llk_sng[b], sng[b], s_slot = end, v, c
            st = int(fit["status"][b, c])
            if (st & capi.DMX_SHARE_INTERIOR) and not (st & capi.DMX_SHARE_NONFINITE) and (d_slot < 0 or fit["ll"][b, c] > llk_dbl[b]):
                llk_dbl[b], d_slot = fit["ll"][b, c], c
        best[b] = d_slot if d_slot >= 0 else s_slot
    with np.errstate(invalid="ignore"):
        is_dbl = (llk_dbl - llk_sng) > CALL_MARGIN
    return dict(llk_sng=llk_sng, sng=sng, llk_dbl=llk_dbl, best=best, is_dbl=is_dbl)


def oriented(v1: int, v2: int, alpha: float):
    """(major, minor, share of the minor donor): the first-named donor is the one with the larger share (v1 on a tie)."""
    return (int(v2), int(v1), 1.0 - alpha) if alpha > 0.5 else (int(v1), int(v2), alpha)


def wald(alpha: float, d2: float):
    """(SE, LO, HI) = 1 / sqrt(-LL''), alpha -+ 1.96 SE clipped to [0, 1]; NaNs unless LL'' < 0."""
    if not (np.isfinite(d2) and d2 < 0.0):
        return np.nan, np.nan, np.nan
    se = 1.0 / math.sqrt(-d2)
    return se, max(0.0, alpha - 1.96 * se), min(1.0, alpha + 1.96 * se)


def status_text(status: int) -> str:
    return ",".join(n for bit, n in STATUS_NAMES if status & bit) or "."


def _num(x, fmt: str) -> str:
    return format(float(x), fmt) if np.isfinite(x) else "NA"


def call_rows(sample_ids: Sequence[str], cand: np.ndarray, pick: np.ndarray, scan: np.ndarray, fit: dict, dec: dict, sng1: np.ndarray):
    """Per barcode the tuple of `.share.tsv`'s columns after BEST, values not yet formatted:
    (CALL, DONOR1, DONOR2, ALPHA, SE, LO, HI, LLK.SNG, LLK.HALF, LLK.HAT, LLR, Z.SCAN, N.EVAL, STATUS, N.SNP, N.READ)."""
    z = scan_z(scan)
    rows = []
    for b in range(cand.shape[0]):
        c = int(dec["best"][b])
        if c < 0:
            name = sample_ids[int(sng1[b])] if sng1[b] >= 0 else "NA"
            rows.append((f"SNG-{name}", "NA", "NA", np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, 0, 0, 0, 0))
            continue
        d1, d2, al = oriented(cand[b, c, 0], cand[b, c, 1], float(fit["alpha"][b, c]))
        se, lo, hi = wald(al, float(fit["d2"][b, c]))
        if dec["is_dbl"][b]:
            call = f"DBL-{sample_ids[d1]}-{sample_ids[d2]}-{al:.3f}"
        else:
            call = f"SNG-{sample_ids[int(dec['sng'][b])]}"
        zs = z[b, pick[b, c, 0], pick[b, c, 1]] if pick[b, c, 0] >= 0 else np.nan
        rows.append((call, sample_ids[d1], sample_ids[d2], al, se, lo, hi, dec["llk_sng"][b], fit["llp"][b, c], fit["ll"][b, c],
                     dec["llk_dbl"][b] - dec["llk_sng"][b], zs, int(fit["n_eval"][b, c]), int(fit["status"][b, c]), int(fit["n_snp"][b, c]),
                     int(fit["n_read"][b, c])))
    return rows


def write_share_tsv(path: str, barcodes: Sequence[str], best: Sequence[str], has_row: np.ndarray, rows) -> None:
    order = sorted(np.flatnonzero(has_row), key=lambda k: barcodes[k].encode())
    with open(path, "w") as f:
        f.write(SHARE_HEADER)
        for k in order:
            r = rows[k]
            f.write(f"{barcodes[k]}\t{best[k]}\t{r[0]}\t{r[1]}\t{r[2]}\t{_num(r[3], '.4f')}\t{_num(r[4], '.4f')}\t{_num(r[5], '.4f')}\t{_num(r[6], '.4f')}\t"
                    f"{_num(r[7], '.5f')}\t{_num(r[8], '.5f')}\t{_num(r[9], '.5f')}\t{_num(r[10], '.5f')}\t{_num(r[11], '.4f')}\t{r[12]}\t"
                    f"{status_text(r[13])}\t{r[14]}\t{r[15]}\n")


def write_scan_tsv(path: str, barcodes: Sequence[str], sample_ids: Sequence[str], has_row: np.ndarray, anchors: np.ndarray, pick: np.ndarray,
                   scan: np.ndarray) -> None:
    order = sorted(np.flatnonzero(has_row), key=lambda k: barcodes[k].encode())
    z = scan_z(scan)
    with open(path, "w") as f:
        f.write(SCAN_HEADER)
        for k in order:
            for t, v in pick[k]:
                if t < 0:
                    continue
                ll, d1, d2 = scan[k, t, v]
                f.write(f"{barcodes[k]}\t{sample_ids[int(anchors[k, t])]}\t{sample_ids[int(v)]}\t{_num(z[k, t, v], '.4f')}\t{_num(ll, '.5f')}\t"
                        f"{_num(d1, '.5f')}\t{_num(d2, '.5f')}\n")


def share_run(store_or_pileup, g: np.ndarray, sample_ids: Sequence[str], out_prefix: str, best: Optional[str] = None, anchors: int = 1,
              top: int = 4, rho=None, ambient="reads", tol: float = 1e-6, max_iter: int = 30, start: float = 0.5,
              alphas: Sequence[float] = (0.0, 0.5), barcodes: Optional[Sequence[str]] = None, device: int = 0,
              mode: int = capi.DMX_MODE_STRICT, **demuxlet_run_kwargs):
    """Scan, fit and call every barcode of `best` (a `.best` path) against genotype matrix g.  Without `best`, the unchanged demuxlet_run
    writes <out_prefix>.best/.single/.sing2 first.  `rho` (None = no soup) is a per-barcode soup fraction [B]; `ambient` is then "reads",
    "genotypes", "census" or an array of n_snps ALT frequencies.  `store_or_pileup` is a Store, or a HostPileup with barcodes=... as for
    demuxlet_run.  Writes <out_prefix>.share.tsv and .share_scan.tsv; returns a dict with the `.best` rows, anchors, the scan, cand, pick,
    the fit, the decision, the rows written, the engine's share_info and the soup profile."""
    from . import ambient as amb_mod
    g = np.ascontiguousarray(g, dtype=np.float32)
    if not 1 <= int(anchors) <= MAX_ANCHORS:
        raise ValueError(f"anchors: 1 to {MAX_ANCHORS}, not {anchors}")
    if not 1 <= int(top) <= MAX_CAND - 1:
        raise ValueError(f"top: 1 to {MAX_CAND - 1}, not {top}")
    if not (tol > 0.0 and np.isfinite(tol)):
        raise ValueError("tol must be a positive number")
    if not 1 <= int(max_iter) <= 200:
        raise ValueError(f"max_iter: 1 to 200, not {max_iter}")
    if not 0.0 < start < 1.0:
        raise ValueError("start must be in (0, 1)")
    if isinstance(ambient, str) and ambient not in ("reads", "genotypes", "census"):
        raise ValueError(f"ambient: 'reads', 'genotypes', 'census' or an array, not {ambient!r}")
    if isinstance(store_or_pileup, engine.HostPileup):
        pl = store_or_pileup
        if barcodes is None:
            raise ValueError("share_run: a HostPileup needs barcodes=")
    else:
        pl, barcodes = store_or_pileup.freeze(), store_or_pileup.barcodes()
    V = len(sample_ids)
    if g.ndim != 3 or g.shape[0] != pl.n_snps or g.shape[1] != V or g.shape[2] != 3:
        raise ValueError(f"genotype matrix {g.shape} for {pl.n_snps} SNPs and {V} samples")
    if not 2 <= V <= MAX_SAMPLES:
        raise ValueError(f"{V} samples: the scan takes 2 to {MAX_SAMPLES}")
    if rho is not None:
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        if rho.shape != (pl.n_cells,) or not np.all((rho >= 0.0) & (rho <= 1.0)):
            raise ValueError(f"rho: {pl.n_cells} values in [0, 1]")
        if not isinstance(ambient, str):
            ambient = amb_mod.check_ambient(ambient, pl.n_snps)
    if best is None:
        engine.demuxlet_run(pl, g, sample_ids, alphas, out_prefix, barcodes=barcodes, device=device, mode=mode, **demuxlet_run_kwargs)
        best = out_prefix + ".best"
    rows = amb_mod.read_best_rows(best, sample_ids, barcodes)
    eng = engine.Engine(V, alphas, device=device, mode=mode)
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        a = None
        if rho is not None:
            a = amb_mod._ambient_builder(ambient, eng, g, lambda: refine.assignments_from_best(best, sample_ids, barcodes)) if isinstance(ambient, str) else ambient
        eng.run_singlet()
        llks, _ = eng.get_singlet()
        anc = anchors_from_singlet(llks, int(anchors))
        anc[~rows.has_row] = -1
        scan, _, _ = eng.share_scan(anc, rho, a)
        cand, pick = select_candidates(scan, anc, int(top), rows.dbl1, rows.dbl2)
        fit = eng.share_fit(cand, rho, a, start=start, tol=tol, max_iter=int(max_iter), probe=0.5)
        info = eng.share_info()
    finally:
        eng.close()
    dec = decide(fit, cand)
    out_rows = call_rows(sample_ids, cand, pick, scan, fit, dec, rows.sng1)
    write_share_tsv(out_prefix + ".share.tsv", barcodes, rows.best, rows.has_row, out_rows)
    write_scan_tsv(out_prefix + ".share_scan.tsv", barcodes, sample_ids, rows.has_row, anc, pick, scan)
    return dict(rows=rows, anchors=anc, scan=scan, cand=cand, pick=pick, fit=fit, decision=dec, calls=out_rows, info=info, ambient=a)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.share",
                                 description="unequal doublets: scan all partners of a barcode's best singlets and fit a continuous mixing share")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.share.tsv, <out>.share_scan.tsv (and <out>.best/... without --best)")
    ap.add_argument("--best", help="a .best of this pileup (default: run the demultiplexing pass first)")
    ap.add_argument("--anchors", type=int, default=1, help=f"best singlets per barcode whose partners are scanned, 1..{MAX_ANCHORS} (default 1)")
    ap.add_argument("--top", type=int, default=4, help=f"partners of highest z whose share is fitted, 1..{MAX_CAND - 1} (default 4)")
    ap.add_argument("--ambient-tsv", help="<x>.ambient.tsv of an ambient.py run: its RHO per barcode is the soup fraction of every hypothesis")
    ap.add_argument("--ambient", choices=("reads", "genotypes", "census"), default=None,
                    help="soup ALT frequency, as for ambient.py (default reads); needs --ambient-tsv")
    ap.add_argument("--tol", type=float, default=1e-6, help="the iteration stops when a step is at most this (default 1e-6)")
    ap.add_argument("--max-iter", type=int, default=30, help="most evaluations inside the bracket, 1..200 (default 30)")
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.0, 0.5], help="doublet grid of the demultiplexing pass (default 0 0.5)")
    ap.add_argument("--fast", action="store_true", help="DMX_MODE_FAST for the demultiplexing pass")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    if not 1 <= a.anchors <= MAX_ANCHORS:
        ap.error(f"--anchors must be in [1, {MAX_ANCHORS}]")
    if not 1 <= a.top <= MAX_CAND - 1:
        ap.error(f"--top must be in [1, {MAX_CAND - 1}]")
    if not (a.tol > 0.0 and np.isfinite(a.tol)):
        ap.error("--tol must be a positive number")
    if not 1 <= a.max_iter <= 200:
        ap.error("--max-iter must be in [1, 200]")
    if a.ambient is not None and a.ambient_tsv is None:
        ap.error("--ambient needs --ambient-tsv")
    if a.ambient is None:
        a.ambient = "reads"
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    from . import fit as fit_mod
    a = parse_args(argv)
    d = refine.read_pileup_txt(a.pileup)
    rho = fit_mod.read_rho_tsv(a.ambient_tsv, d.barcodes) if a.ambient_tsv else None
    r = share_run(d.pileup, d.g, d.sample_ids, a.out, best=a.best, anchors=a.anchors, top=a.top, rho=rho, ambient=a.ambient, tol=a.tol,
                  max_iter=a.max_iter, alphas=a.alpha, barcodes=d.barcodes, device=a.gpu,
                  mode=capi.DMX_MODE_FAST if a.fast else capi.DMX_MODE_STRICT)
    n = int(r["rows"].has_row.sum())
    n_dbl = int((r["decision"]["is_dbl"] & r["rows"].has_row).sum())
    print(f"{n} barcodes; {n_dbl} DBL- by the fitted share ({sum(b.startswith('DBL-') for b in r['rows'].best)} in the .best)", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
