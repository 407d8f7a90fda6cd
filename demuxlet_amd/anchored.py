"""Anchored doublet search: demultiplex pools of hundreds of donors without the V x V x A doublet grid.

Per barcode the engine keeps the whole singlet column, takes the T best singlets as anchors and scores every donor of the panel as the
partner of every anchor, in both orders (Engine.doublet_anchored / dmx_engine_doublet_anchored): about (2T + 1) V (A - 1) + V A entries
where the full grid has V V A, each bit for bit the STRICT grid's entry.  `.single` is K1's, `.sing2` / `.best` come from the existing
writer over the singlet column, llks00 and the per-barcode records, `.anchors.tsv` lists the anchors.  What the restriction costs: the
best pair is found whenever one of its donors is an anchor, and PRB.DBL, summed over the evaluated pairs only, is a lower bound of the
reference's.  `--verify N` runs the full STRICT grid on N barcodes and writes both answers side by side.

    python -m demuxlet_amd.anchored --pileup <x>.pileup.txt --out <prefix> [--anchors T] [--alpha A ...] [--doublet-prior P]
        [--min-total/--min-uniq/--min-snp N] [--no-arbiter] [--verify N] [--seed S] [--gpu G]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
from typing import Optional, Sequence

import numpy as np

from . import capi, dist, engine, refine

MAX_ANCHORS = 8             # dmx_engine_doublet_anchored's limit
CHECK_HEADER = "BARCODE\tBEST.FULL\tBEST.ANCHORED\tSAME.CALL\tSAME.PAIR\tPRB.DBL.FULL\tPRB.DBL.ANCHORED\n"


def check_n_anchor(n_anchor: int, n_samples: int) -> int:
    """dmx_engine_doublet_anchored's rule: 1 <= T <= min(8, V)."""
    T = int(n_anchor)
    if T < 1 or T > MAX_ANCHORS:
        raise ValueError(f"anchors: {T} is not in [1, {MAX_ANCHORS}]")
    if T > n_samples:
        raise ValueError(f"anchors: {T} anchors for {n_samples} samples")
    return T


def check_alphas(alphas: Sequence[float]) -> np.ndarray:
    al = np.asarray(alphas, dtype=np.float64)
    if al.ndim != 1 or len(al) < 2:
        raise ValueError("alpha: the anchored search needs at least two alphas (the first is the singlet column's)")
    if not np.all((al >= 0.0) & (al <= 1.0)):
        raise ValueError("alpha: every value must be in [0, 1]")
    return al


def entries_per_barcode(anchors: np.ndarray, V: int, A: int) -> np.ndarray:
    """N.ENTRY: entries evaluated for each barcode — column 0 and llks00, and both orders of every used anchor's partners."""
    used = (np.asarray(anchors) >= 0).sum(axis=1)
    return V * A + A + used * (V - 1) * 2 * (A - 1)


def write_anchors_tsv(path: str, barcodes: Sequence[str], sample_ids: Sequence[str], n_snp: np.ndarray, anchors: np.ndarray, A: int) -> None:
    """One row per barcode with a covered SNP, in ascending byte-wise barcode order (the writers' order); `.` for an unused anchor."""
    anchors = np.asarray(anchors)
    T = anchors.shape[1]
    n_ent = entries_per_barcode(anchors, len(sample_ids), A)
    order = sorted(np.flatnonzero(np.asarray(n_snp) > 0), key=lambda k: barcodes[k].encode())
    with open(path, "w") as f:
        f.write("BARCODE\tN.SNP\t" + "\t".join(f"ANCHOR.{t + 1}" for t in range(T)) + "\tN.ENTRY\n")
        for k in order:
            names = "\t".join(sample_ids[int(a)] if a >= 0 else "." for a in anchors[k])
            f.write(f"{barcodes[k]}\t{int(n_snp[k])}\t{names}\t{int(n_ent[k])}\n")


def read_best_columns(path: str) -> dict:
    """{barcode: (BEST, PRB.DBL text)} of a `.best`."""
    out = {}
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        ib, ibest, ip = head.index("BARCODE"), head.index("BEST"), head.index("PRB.DBL")
        for line in f:
            t = line.rstrip("\n").split("\t")
            out[t[ib]] = (t[ibest], t[ip])
    return out


def same_pair(rec_full, rec_anch, alphas: Sequence[float]) -> bool:
    """The two records name the same best doublet entry (j, k, n).  At alpha[n] = 0.5 (j, k) and (k, j) are one hypothesis, whose order
    the arbiter settles, and the order is ignored; at any other alpha they are different entries with different likelihoods."""
    n = int(rec_full["n_best"])
    if n != int(rec_anch["n_best"]):
        return False
    f, a = (int(rec_full["j_best"]), int(rec_full["k_best"])), (int(rec_anch["j_best"]), int(rec_anch["k_best"]))
    return f == a or (n >= 0 and alphas[n] == 0.5 and f == a[::-1])


def prb_dbl(rec) -> float:
    return float(rec["sum_double"] / (rec["sum_single"] + rec["sum_double"]))


def write_check_tsv(path: str, barcodes: Sequence[str], best_full: Sequence[str], best_anch: Sequence[str], same_pairs: Sequence[bool],
                    prb_full: Sequence[float], prb_anch: Sequence[float]) -> dict:
    """<prefix>.anchored_check.tsv over the verified barcodes, in ascending byte-wise barcode order.  Returns the three counts."""
    order = sorted(range(len(barcodes)), key=lambda k: barcodes[k].encode())
    n_call = n_pair = 0
    with open(path, "w") as f:
        f.write(CHECK_HEADER)
        for k in order:
            sc, sp = int(best_full[k] == best_anch[k]), int(bool(same_pairs[k]))
            n_call += sc; n_pair += sp
            f.write(f"{barcodes[k]}\t{best_full[k]}\t{best_anch[k]}\t{sc}\t{sp}\t{prb_full[k]:.6g}\t{prb_anch[k]:.6g}\n")
    return dict(n_verified=len(order), n_same_call=n_call, n_same_pair=n_pair)


def _free_device_bytes(gpu: int) -> Optional[int]:
    """Free bytes of the device, or None without torch (--verify then says that it could not size its sample)."""
    try:
        import torch
    except ImportError:
        return None
    return int(torch.cuda.mem_get_info(gpu)[0])


def verify_cells(n_pairs: np.ndarray, n: int, seed: int, grid_bytes_per_cell: int, free_bytes: Optional[int]):
    """The barcodes --verify takes: n covered ones drawn without replacement by a seeded generator — fewer if their grids would not fit
    half of the free device memory.  Returns (cell ids, whether the count was cut)."""
    covered = np.flatnonzero(np.asarray(n_pairs) > 0)
    want = min(int(n), len(covered))
    cut = False
    if free_bytes is not None and want * grid_bytes_per_cell > free_bytes // 2:
        want, cut = max(0, int((free_bytes // 2) // grid_bytes_per_cell)), True
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(covered, size=want, replace=False)) if want > 0 else np.zeros(0, dtype=np.int64), cut


def anchored_run(store_or_pileup, g: np.ndarray, sample_ids: Sequence[str], alphas: Sequence[float] = (0.0, 0.5), out_prefix: str = "anchored",
                 n_anchor: int = 2, doublet_prior: float = 0.5, min_total: int = 0, min_uniq: int = 0, min_snp: int = 0, arbiter: bool = True,
                 verify: int = 0, seed: int = 0, gpu: int = 0, barcodes: Optional[Sequence[str]] = None):
    """K1 and the anchored doublet pass over the pileup; writes <out_prefix>.single / .sing2 / .best / .anchors.tsv and, with verify > 0,
    <out_prefix>.anchored_check.tsv.  `store_or_pileup` is a Store, or a HostPileup with barcodes=... as for demuxlet_run.  Returns a dict
    with the anchored arrays, the info and the verification counts."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    al = check_alphas(alphas)
    if isinstance(store_or_pileup, engine.HostPileup):
        pl = store_or_pileup
        if barcodes is None:
            raise ValueError("anchored_run: a HostPileup needs barcodes=")
    else:
        pl, barcodes = store_or_pileup.freeze(), store_or_pileup.barcodes()
    V, A = len(sample_ids), len(al)
    if g.ndim != 3 or g.shape[0] != pl.n_snps or g.shape[1] != V or g.shape[2] != 3:
        raise ValueError(f"genotype matrix {g.shape} for {pl.n_snps} SNPs and {V} samples")
    T = check_n_anchor(n_anchor, V)
    if verify < 0:
        raise ValueError("verify: a count of barcodes, 0 = none")
    eng = engine.Engine(V, al, doublet_prior, device=gpu)
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        eng.run_singlet()
        llks, llk0s = eng.get_singlet()
        eng.doublet_anchored(T)
        res = eng.get_anchored()
        info = eng.anchored_info()
    finally:
        eng.close()
    sing = np.ascontiguousarray(res["c0"][:, :, 0])
    fa = engine.FinalArgs(barcodes, sample_ids, al, doublet_prior, pl.rd_totl, pl.rd_pass, pl.rd_uniq, pl.n_snp_per_cell, min_total, min_uniq,
                          min_snp, False)
    engine.write_single(fa, llks, llk0s, out_prefix + ".single")
    try:
        engine.write_doublet_summary(fa, sing, res["llks00"], res["summary"], out_prefix, tie_pileup=pl if arbiter else None,
                                     tie_g=g if arbiter else None)
    except capi.DmxError as ex:
        if arbiter and "near-tie-flagged" in str(ex):
            raise capi.DmxError(ex.code, str(ex).split(": ", 1)[-1] + " (the anchored search has no grids to pass: with the arbiter on, near-tie "
                                "barcodes are re-evaluated on the host; --no-arbiter / arbiter=False writes the device's own order instead)") from ex
        raise
    write_anchors_tsv(out_prefix + ".anchors.tsv", barcodes, sample_ids, pl.n_snp_per_cell, res["anchors"], A)
    out = dict(res, sing=sing, llks=llks, llk0s=llk0s, info=info, check=None)
    if verify > 0:
        free_b = _free_device_bytes(gpu)
        if free_b is None:
            print("anchored: --verify: torch is not importable, so the free device memory is unknown and the sample is not cut to fit it", file=sys.stderr)
        cells, cut = verify_cells(res["summary"]["n_pairs"], verify, seed, V * V * A * 8, free_b)
        if cut:
            print(f"anchored: --verify {verify}: the full grids of {len(cells)} barcodes fit the free device memory; verifying those", file=sys.stderr)
        out["check"] = _verify(pl, g, barcodes, sample_ids, al, doublet_prior, min_total, min_uniq, min_snp, arbiter, gpu, cells, res, out_prefix)
        c = out["check"]
        print(f"anchored: verified {c['n_verified']} barcodes against the full grid: {c['n_same_call']} same call, {c['n_same_pair']} same best pair",
              file=sys.stderr)
    return out


def _verify(pl, g, barcodes, sample_ids, al, doublet_prior, min_total, min_uniq, min_snp, arbiter, gpu, cells, res, out_prefix) -> dict:
    V = len(sample_ids)
    sub = dist.slice_pileup(pl, cells)
    bcs = [barcodes[int(c)] for c in cells]
    full = engine.Engine(V, al, doublet_prior, device=gpu, mode=capi.DMX_MODE_STRICT)
    try:
        full.set_genotypes(g)
        full.set_pileup(sub)
        full.run()
        _, l00, summ = full.get_doublet(want_grid=False)
        sing = full.get_sing()
        near = engine.near_tie_cells(summ)
        grids = full.get_cell_grids(near)
    finally:
        full.close()
    fa = engine.FinalArgs(bcs, sample_ids, al, doublet_prior, sub.rd_totl, sub.rd_pass, sub.rd_uniq, sub.n_snp_per_cell, min_total, min_uniq,
                          min_snp, False)
    with tempfile.TemporaryDirectory(dir=os.path.dirname(os.path.abspath(out_prefix))) as td:
        pre = os.path.join(td, "full")
        engine.write_doublet_summary(fa, sing, l00, summ, pre, tie_pileup=sub if arbiter else None, tie_g=g if arbiter else None,
                                     cell_grids={int(c): gr for c, gr in zip(near, grids)})
        best_f = read_best_columns(pre + ".best")
    best_a = read_best_columns(out_prefix + ".best")
    asum = res["summary"][cells]
    keep = [k for k, b in enumerate(bcs) if b in best_f and b in best_a]          # (the --min-* filters drop the same rows from both)
    return write_check_tsv(out_prefix + ".anchored_check.tsv", [bcs[k] for k in keep], [best_f[bcs[k]][0] for k in keep],
                           [best_a[bcs[k]][0] for k in keep], [same_pair(summ[k], asum[k], al) for k in keep],
                           [prb_dbl(summ[k]) for k in keep], [prb_dbl(asum[k]) for k in keep])


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.anchored",
                                 description="anchored doublet search: demultiplex wide donor panels without the V x V doublet grid")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.single / .sing2 / .best / .anchors.tsv")
    ap.add_argument("--anchors", type=int, default=2, metavar="T", help=f"best singlets kept as anchors per barcode, 1..{MAX_ANCHORS} (default 2)")
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.0, 0.5], help="doublet grid, at least two values (default 0 0.5)")
    ap.add_argument("--doublet-prior", type=float, default=0.5)
    ap.add_argument("--min-total", type=int, default=0)
    ap.add_argument("--min-uniq", type=int, default=0)
    ap.add_argument("--min-snp", type=int, default=0)
    ap.add_argument("--no-arbiter", action="store_true", help="write the device's own order of a doublet's donors; near-tie barcodes are not re-evaluated")
    ap.add_argument("--verify", type=int, default=0, metavar="N", help="run the full STRICT grid on N barcodes and write <out>.anchored_check.tsv")
    ap.add_argument("--seed", type=int, default=0, help="seed of --verify's choice of barcodes")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    try:
        if a.anchors < 1 or a.anchors > MAX_ANCHORS:
            raise ValueError(f"--anchors {a.anchors} is not in [1, {MAX_ANCHORS}]")
        check_alphas(a.alpha)
        if not (0.0 <= a.doublet_prior <= 1.0):
            raise ValueError("--doublet-prior must be in [0, 1]")
        if a.verify < 0:
            raise ValueError("--verify: a count of barcodes")
    except ValueError as ex:
        ap.error(str(ex))
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    d = refine.read_pileup_txt(a.pileup)
    r = anchored_run(d.pileup, d.g, d.sample_ids, a.alpha, a.out, n_anchor=a.anchors, doublet_prior=a.doublet_prior, min_total=a.min_total,
                     min_uniq=a.min_uniq, min_snp=a.min_snp, arbiter=not a.no_arbiter, verify=a.verify, seed=a.seed, gpu=a.gpu,
                     barcodes=d.barcodes)
    inf = r["info"]
    print(f"anchored: {inf['n_cells']} barcodes x {inf['n_samples']} samples, {inf['n_anchor']} anchors: {inf['n_entries']} entries in "
          f"{inf['col_ms'] + inf['pair_ms'] + inf['reduce_ms']:.3f} ms, {inf['result_bytes']} result bytes", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
