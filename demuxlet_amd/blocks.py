"""Block-resolved likelihoods: jackknife errors and leave-one-block-out calls.

Every call is a sum of per-SNP terms over the whole genome, and the printed total does not say where along the genome it came from.
The engine (Engine.block_llk, dmx_engine_block_llk) gives every barcode's singlet column, llks00 and a few chosen
grid entries summed per genomic BLOCK — the STRICT grid's own terms, so one block is the whole grid bit for bit.  From those sums, per
barcode and for the two differences LLR.SNG = SNG.1ST - SNG.2ND and LLR.DBL = best doublet - SNG.1ST (the donors and the doublet pair
are the `.best` row's; the doublet is the better of its two orders), with C the blocks the barcode covers, m = |C|, d_g a difference's
value in block g and D its sum over C:

  SE = sqrt(m / (m - 1) * sum_C (d_g - D / m)^2), the delete-one-block jackknife of a total (NA for m < 2);  Z = D / SE.
  TOP.BLOCK / TOP.SHARE: the block with the largest d_g of the difference that decides BEST (LLR.DBL for DBL-, else LLR.SNG), and d_g / D.
  LOO.MIN: the minimum over g of D - d_g of that difference.
  For each g in C the reference's DBL / SNG / AMB rule (cmd_cram_demuxlet.cpp:837-857) is applied again to the sums without block g:
  the singlet column is ranked again over all donors, the doublet pair stays fixed.  N.LOO.SAME counts the deletions that give BEST's
  type and donors again, LOO.CALL is the commonest call that differs (`.` when none does), and FLAG is LOWN for m < --min-blocks,
  FRAGILE when a deletion changes the call, otherwise STABLE.

Per (donor d, block g), over the barcodes with BEST = SNG-d that cover g: LLR.2ND = the sum of col[d] minus each cell's own SNG.2ND in
the block, N.OTHER = the cells whose best column inside the block alone is not d, BEST.OTHER the commonest such column, and FLAG = SWAP?
when N.CELL >= --min-cells and N.OTHER > N.CELL / 2 — sample columns exchanged in one region only, which the whole-genome calls outvote.

  <prefix>.blocks.tsv        BLOCK RID START END N.SNP
  <prefix>.block_calls.tsv   BARCODE BEST N.BLOCK LLR.SNG SE.SNG Z.SNG LLR.DBL SE.DBL Z.DBL TOP.BLOCK TOP.SHARE LOO.MIN N.LOO.SAME LOO.CALL FLAG
  <prefix>.block_donors.tsv  SM_ID BLOCK N.CELL N.SNP LLR.2ND N.OTHER BEST.OTHER FLAG

Blocks are runs of SNPs in file order that never cross a change of RID: --blocks N gives every chromosome max(1, round(N x its share
of the SNPs)) runs of equal SNP count, --block-bp N windows of N bases from the chromosome's first SNP, --by-chrom one per chromosome.
Without --best the unchanged demultiplexing pass writes <prefix>.best/.single/.sing2 first; `.best` is never changed.
Limits: the doublet pair is fixed under deletion and not searched again; --min-blocks and --min-cells are knobs, not tests; blocks are
runs in SNP order, not LD blocks; the jackknife of a total is conservative (too wide) for blocks of unequal size; no soup term; one GPU.

    python -m demuxlet_amd.blocks --pileup <x>.pileup.txt --out <prefix> [--best <x>.best] [--blocks 40 | --block-bp N | --by-chrom]
        [--min-blocks 5] [--min-cells 10] [--alpha A ...] [--fast] [--gpu G]"""
from __future__ import annotations

import argparse
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

SNG, DBL, AMB = 0, 1, 2
BLOCKS_HEADER = "BLOCK\tRID\tSTART\tEND\tN.SNP\n"
CALLS_HEADER = ("BARCODE\tBEST\tN.BLOCK\tLLR.SNG\tSE.SNG\tZ.SNG\tLLR.DBL\tSE.DBL\tZ.DBL\tTOP.BLOCK\tTOP.SHARE\tLOO.MIN\tN.LOO.SAME\tLOO.CALL\t"
                "FLAG\n")
DONORS_HEADER = "SM_ID\tBLOCK\tN.CELL\tN.SNP\tLLR.2ND\tN.OTHER\tBEST.OTHER\tFLAG\n"


def make_blocks(snps: Sequence, n_blocks: Optional[int] = 40, block_bp: Optional[int] = None, by_chrom: bool = False):
    """(ids int32 [S], table) for snps = (rid, pos, ...) per SNP in file order.  Blocks are runs of SNPs that never cross a change of
    RID; ids are 0, 1, .. in file order (non-decreasing); table rows are (block, rid, first pos, last pos, SNPs).  by_chrom: one block
    per chromosome run; block_bp: windows of block_bp bases from the run's first SNP (empty windows get no id); otherwise every run gets
    max(1, round(n_blocks x its share of the SNPs)) blocks of equal SNP count (to within one)."""
    S = len(snps)
    rid = np.array([s[0] for s in snps], dtype=np.int64)
    pos = np.array([s[1] for s in snps], dtype=np.int64)
    if not by_chrom and block_bp is None and (n_blocks is None or int(n_blocks) < 1):
        raise ValueError(f"n_blocks: at least 1, not {n_blocks}")
    if block_bp is not None and int(block_bp) < 1:
        raise ValueError(f"block_bp: at least 1, not {block_bp}")
    starts = np.concatenate([[0], np.flatnonzero(np.diff(rid) != 0) + 1, [S]]) if S else np.array([0], dtype=np.int64)
    ids = np.zeros(S, dtype=np.int32)
    nxt = 0
    for a, b in zip(starts[:-1], starts[1:]):
        n = int(b - a)
        if by_chrom:
            part = np.zeros(n, dtype=np.int64)
        elif block_bp is not None:
            w = (pos[a:b] - pos[a]) // int(block_bp)
            part = np.concatenate([[0], np.cumsum(np.diff(w) != 0)])
        else:
            k = min(n, max(1, int(round(int(n_blocks) * n / S))))
            part = (np.arange(n) * k) // n
        ids[a:b] = nxt + part
        nxt += int(part[-1]) + 1
    table = []
    if S:
        first = np.concatenate([[0], np.flatnonzero(np.diff(ids) != 0) + 1])
        last = np.concatenate([first[1:], [S]]) - 1
        table = [(int(ids[f]), int(rid[f]), int(pos[f]), int(pos[l]), int(l - f + 1)) for f, l in zip(first, last)]
    return ids, table


def write_blocks_tsv(path: str, table: Sequence) -> None:
    with open(path, "w") as f:
        f.write(BLOCKS_HEADER)
        for b, rid, start, end, n in table:
            f.write(f"{b}\t{rid}\t{start}\t{end}\t{n}\n")


@dataclass
class BestRows:
    """What the block statistics read of a `.best`, by cell id (kind = -1 and best = "" without a row)."""
    best: List[str]
    kind: np.ndarray         # int8 [B]: SNG, DBL, AMB or -1
    sng1: np.ndarray         # int32 [B]: SNG.1ST, SNG.2ND, DBL.1ST, DBL.2ND as sample indices
    sng2: np.ndarray
    dbl1: np.ndarray
    dbl2: np.ndarray
    n_alpha: np.ndarray      # int32 [B]: the index of ALPHA in the alpha grid

    @property
    def has_row(self) -> np.ndarray:
        return self.kind >= 0


def empty_rows(B: int) -> BestRows:
    neg = lambda: np.full(B, -1, dtype=np.int32)
    return BestRows([""] * B, np.full(B, -1, dtype=np.int8), neg(), neg(), neg(), neg(), np.zeros(B, dtype=np.int32))


def read_best_rows(path: str, sample_ids: Sequence[str], barcodes: Sequence[str], alphas: Sequence[float]) -> BestRows:
    smap = {s: j for j, s in enumerate(sample_ids)}
    cmap = {b: c for c, b in enumerate(barcodes)}
    al = np.asarray(alphas, dtype=np.float64)
    out = empty_rows(len(barcodes))
    need = ("BARCODE", "BEST", "SNG.1ST", "SNG.2ND", "DBL.1ST", "DBL.2ND", "ALPHA")
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
            best = t[col["BEST"]]
            if best[:4] not in ("SNG-", "DBL-", "AMB-"):
                raise ValueError(f"{path}: BEST {best!r} is not SNG-, DBL- or AMB-")
            idx = []
            for n in ("SNG.1ST", "SNG.2ND", "DBL.1ST", "DBL.2ND"):
                j = smap.get(t[col[n]])
                if j is None:
                    raise ValueError(f"{path}: sample {t[col[n]]!r} not in this job")
                idx.append(j)
            a = float(t[col["ALPHA"]])
            n_a = int(np.argmin(np.abs(al - a)))
            if abs(al[n_a] - a) > 5.1e-4:                      # ALPHA is printed with three decimals
                raise ValueError(f"{path}: ALPHA {a} of {t[col['BARCODE']]!r} is not on the alpha grid {list(al)}")
            out.best[c] = best
            out.kind[c] = ("SNG-", "DBL-", "AMB-").index(best[:4])
            out.sng1[c], out.sng2[c], out.dbl1[c], out.dbl2[c] = idx
            out.n_alpha[c] = n_a
    return out


def extras_from_rows(rows: BestRows) -> np.ndarray:
    """extra[B][2][3] for Engine.block_llk: the `.best` row's doublet (DBL.1ST, DBL.2ND, its alpha index) and the same pair in the other
    order; both slots unused for a barcode without a row."""
    B = len(rows.best)
    ex = np.zeros((B, 2, 3), dtype=np.int32)
    ex[:, 0, 0], ex[:, 0, 1] = rows.dbl1, rows.dbl2
    ex[:, 1, 0], ex[:, 1, 1] = rows.dbl2, rows.dbl1
    ex[:, :, 2] = rows.n_alpha[:, None]
    ex[~rows.has_row] = (-1, 0, 0)
    return ex


def _seq_sum(x: np.ndarray, axis: int) -> np.ndarray:
    """The serial left-to-right sum along an axis (np.sum adds pairwise, which rounds otherwise)."""
    if x.shape[axis] == 0:
        return np.zeros(np.delete(x.shape, axis), dtype=x.dtype)
    return np.take(np.cumsum(x, axis=axis), -1, axis=axis)


def _pick(a: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """a[b, ..., idx[b]] for every b."""
    ix = idx.reshape((-1,) + (1,) * (a.ndim - 1))
    return np.take_along_axis(a, np.broadcast_to(ix, a.shape[:-1] + (1,)), axis=-1)[..., 0]


def doublet_order(e: np.ndarray, dbl1: np.ndarray, dbl2: np.ndarray) -> np.ndarray:
    """Which of the two orders the reference's scan (:799-814: j, then k ascending, strict <) keeps: e[..., 0] is (dbl1, dbl2) and
    e[..., 1] is (dbl2, dbl1); the scan meets the order with the smaller first donor first and leaves it only for a larger value."""
    first = np.where(dbl1 <= dbl2, 0, 1)
    ef, es = _pick(e, first), _pick(e, 1 - first)
    return np.where(es > ef, 1 - first, first)


def rank_singlets(col: np.ndarray):
    """(SNG.1ST, SNG.2ND) of a column [B][V] by the reference's scan (:746-758): the first maximum, and the first maximum of the rest."""
    s1 = np.argmax(col, axis=1)
    rest = col.copy()
    rest[np.arange(len(col)), s1] = -np.inf
    return s1, np.argmax(rest, axis=1)


def call_rule(col: np.ndarray, e: np.ndarray, dbl1: np.ndarray, dbl2: np.ndarray):
    """The reference's rule (:837-857) on singlet columns col[B][V] and the fixed pair's two orders e[B][2]: (kind, s1, s2, order)."""
    s1, s2 = rank_singlets(col)
    o = doublet_order(e, dbl1, dbl2)
    llk12 = _pick(e, o)
    sing1, sing2 = _pick(col, s1), _pick(col, s2)
    jb, kb = np.where(o == 0, dbl1, dbl2), np.where(o == 0, dbl2, dbl1)
    dbl = (llk12 > _pick(col, jb)) & (llk12 > _pick(col, kb)) & (llk12 > sing1 + 2)
    kind = np.where(dbl, DBL, np.where(sing1 > sing2 + 2, SNG, AMB)).astype(np.int8)
    return kind, s1.astype(np.int32), s2.astype(np.int32), o.astype(np.int32)


def _jackknife(d: np.ndarray, cov: np.ndarray, m: np.ndarray):
    """(D, SE, Z) of a difference d[B][G] over the covered blocks."""
    d = np.where(cov, d, 0.0)
    D = _seq_sum(d, 1)
    mf = m.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        dev = np.where(cov, d - (D / mf)[:, None], 0.0)
        ss = _seq_sum(dev * dev, 1)
        se = np.where(m >= 2, np.sqrt(mf / (mf - 1.0) * ss), np.nan)
        z = D / se
    return D, se, z


def call_label(kind: int, s1: int, s2: int, j: int, k: int, alpha: float, sample_ids: Sequence[str]) -> str:
    """The BEST string of the reference for a call (:839-856)."""
    if kind == DBL:
        return f"DBL-{sample_ids[j]}-{sample_ids[k]}-{alpha:.3f}"
    if kind == SNG:
        return f"SNG-{sample_ids[s1]}"
    return f"AMB-{sample_ids[s1]}-{sample_ids[s2]}-{sample_ids[j]}/{sample_ids[k]}"


def block_calls(res: dict, rows: BestRows, min_blocks: int = 5) -> dict:
    """The per-barcode statistics of the module docstring from Engine.block_llk's dict (col[B][G][V], ext[B][G][2] for
    extras_from_rows(rows), n_snp[B][G]).  Barcodes without a `.best` row get m = 0 and NaN.  loo_call[b] is None or the call
    (kind, s1, s2, order) of the commonest deletion that differs (the first such block in ascending order among equals)."""
    col, ext, n_snp = np.asarray(res["col"]), np.asarray(res["ext"]), np.asarray(res["n_snp"])
    B, G, V = col.shape
    has = rows.has_row
    cov = (n_snp > 0) & has[:, None]
    m = cov.sum(axis=1).astype(np.int32)
    z = np.zeros(B, dtype=np.int64)
    s1, s2 = np.where(has, rows.sng1, z), np.where(has, rows.sng2, z)
    d1, d2 = np.where(has, rows.dbl1, z), np.where(has, rows.dbl2, z)
    t_col, t_ext = _seq_sum(col, 1), _seq_sum(ext, 1)
    o = doublet_order(t_ext, d1, d2)
    c1 = _pick(col, s1)                                                   # [B][G]
    d_sng = c1 - _pick(col, s2)
    d_dbl = _pick(ext, o) - c1
    D_s, se_s, z_s = _jackknife(d_sng, cov, m)
    D_d, se_d, z_d = _jackknife(d_dbl, cov, m)
    is_dbl = rows.kind == DBL
    d_dec = np.where(cov, np.where(is_dbl[:, None], d_dbl, d_sng), -np.inf)
    D_dec = np.where(is_dbl, D_d, D_s)
    top = np.where(m > 0, np.argmax(d_dec, axis=1), -1).astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        d_top = np.where(m > 0, _pick(d_dec, np.maximum(top, 0)), np.nan)
        top_share = d_top / D_dec
        loo_min = np.where(m > 0, np.min(np.where(cov, D_dec[:, None] - d_dec, np.inf), axis=1), np.nan)
    # the rule without each block in turn
    code = np.full((B, G), -1, dtype=np.int64)                            # the differing calls, coded; -1 = same, or not covered
    n_same = np.zeros(B, dtype=np.int32)
    for g in range(G):
        kind, r1, r2, ro = call_rule(t_col - col[:, g], t_ext - ext[:, g], d1, d2)
        same = (kind == rows.kind) & np.where(kind == DBL, True, r1 == s1) & np.where(kind == AMB, r2 == s2, True)
        n_same += (same & cov[:, g])
        a = np.where(kind == DBL, 0, r1).astype(np.int64)                 # a call's donors: SNG s1; DBL the order; AMB s1, s2 and the order
        b = np.where(kind == AMB, r2, 0).astype(np.int64)
        w = np.where(kind == SNG, 0, ro).astype(np.int64)
        code[:, g] = np.where(cov[:, g] & ~same, (kind.astype(np.int64) << 44) | (w << 42) | (a << 21) | b, -1)
    loo_call: List[Optional[Tuple[int, int, int, int]]] = [None] * B
    for b in np.flatnonzero((code >= 0).any(axis=1)):
        cs = code[b][code[b] >= 0]
        vals, first, cnt = np.unique(cs, return_index=True, return_counts=True)
        w = int(vals[np.lexsort((first, -cnt))[0]])
        kind, ro, a, c2 = w >> 44, (w >> 42) & 1, (w >> 21) & 0x1FFFFF, w & 0x1FFFFF
        loo_call[b] = (kind, -1 if kind == DBL else a, c2 if kind == AMB else -1, ro)
    fragile = np.array([c is not None for c in loo_call], dtype=bool)
    flag = np.where(m < int(min_blocks), "LOWN", np.where(fragile, "FRAGILE", "STABLE"))
    return dict(m=m, llr_sng=D_s, se_sng=se_s, z_sng=z_s, llr_dbl=D_d, se_dbl=se_d, z_dbl=z_d, top_block=top, top_share=top_share,
                loo_min=loo_min, n_loo_same=n_same, loo_call=loo_call, flag=flag, order=o.astype(np.int32))


def loo_label(rows: BestRows, b: int, call, alphas: Sequence[float], sample_ids: Sequence[str]) -> str:
    if call is None:
        return "."
    kind, r1, r2, ro = call
    j, k = (rows.dbl1[b], rows.dbl2[b]) if ro == 0 else (rows.dbl2[b], rows.dbl1[b])
    return call_label(kind, r1, r2, int(j), int(k), float(alphas[rows.n_alpha[b]]), sample_ids)


def block_donors(res: dict, rows: BestRows, min_cells: int = 10) -> List[tuple]:
    """[(d, g, N.CELL, N.SNP, LLR.2ND, N.OTHER, BEST.OTHER or -1, flag)] over the (donor, block) pairs that a barcode with BEST = SNG-d
    covers, in (d, g) order.  BEST.OTHER: the commonest best column that is not d (the lowest index among equals)."""
    col, n_snp = np.asarray(res["col"]), np.asarray(res["n_snp"])
    B, G, V = col.shape
    out = []
    for d in range(V):
        cells = np.flatnonzero((rows.kind == SNG) & (rows.sng1 == d))
        for g in range(G):
            sel = cells[n_snp[cells, g] > 0]
            if not len(sel):
                continue
            c = col[sel, g]
            llr = float(_seq_sum(c[:, d] - c[np.arange(len(sel)), rows.sng2[sel]], 0))
            best = np.argmax(c, axis=1)
            other = best[best != d]
            top = int(np.argmax(np.bincount(other, minlength=V))) if len(other) else -1
            swap = len(sel) >= int(min_cells) and 2 * len(other) > len(sel)
            out.append((d, g, len(sel), int(n_snp[sel, g].sum()), llr, len(other), top, "SWAP?" if swap else "."))
    return out


def _num(x, fmt: str) -> str:
    return format(float(x), fmt) if np.isfinite(x) else "NA"


def write_calls_tsv(path: str, barcodes: Sequence[str], sample_ids: Sequence[str], alphas: Sequence[float], rows: BestRows, st: dict) -> dict:
    """One row per barcode of the `.best`, in ascending byte-wise barcode order (the writers' order); returns the count of each FLAG."""
    order = sorted(np.flatnonzero(rows.has_row), key=lambda k: barcodes[k].encode())
    n = {"LOWN": 0, "FRAGILE": 0, "STABLE": 0}
    with open(path, "w") as f:
        f.write(CALLS_HEADER)
        for k in order:
            n[str(st["flag"][k])] += 1
            f.write(f"{barcodes[k]}\t{rows.best[k]}\t{int(st['m'][k])}\t{_num(st['llr_sng'][k], '.4f')}\t{_num(st['se_sng'][k], '.4f')}\t"
                    f"{_num(st['z_sng'][k], '.3f')}\t{_num(st['llr_dbl'][k], '.4f')}\t{_num(st['se_dbl'][k], '.4f')}\t{_num(st['z_dbl'][k], '.3f')}\t"
                    f"{int(st['top_block'][k]) if st['top_block'][k] >= 0 else 'NA'}\t{_num(st['top_share'][k], '.4f')}\t{_num(st['loo_min'][k], '.4f')}\t"
                    f"{int(st['n_loo_same'][k])}\t{loo_label(rows, k, st['loo_call'][k], alphas, sample_ids)}\t{st['flag'][k]}\n")
    return n


def write_donors_tsv(path: str, sample_ids: Sequence[str], table: Sequence[tuple]) -> int:
    """Returns the number of SWAP? rows."""
    with open(path, "w") as f:
        f.write(DONORS_HEADER)
        for d, g, n_cell, n_snp, llr, n_other, top, flag in table:
            f.write(f"{sample_ids[d]}\t{g}\t{n_cell}\t{n_snp}\t{_num(llr, '.4f')}\t{n_other}\t{sample_ids[top] if top >= 0 else '.'}\t{flag}\n")
    return sum(r[7] == "SWAP?" for r in table)


def block_run(store_or_pileup, g: np.ndarray, sample_ids: Sequence[str], out_prefix: str, snps: Optional[Sequence] = None,
              best: Optional[str] = None, n_blocks: Optional[int] = 40, block_bp: Optional[int] = None, by_chrom: bool = False,
              min_blocks: int = 5, min_cells: int = 10, alphas: Sequence[float] = (0.0, 0.5), barcodes: Optional[Sequence[str]] = None,
              device: int = 0, mode: Optional[int] = None, block: Optional[Tuple[np.ndarray, Sequence]] = None, **demuxlet_run_kwargs):
    """Block statistics of every barcode's call in `best` (a `.best` path; without it the unchanged demuxlet_run writes
    <out_prefix>.best/.single/.sing2 first).  `snps` is (rid, pos, ref, alt) per SNP (default: one chromosome, the SNP id as position);
    `block` = (ids, table) overrides make_blocks.  Writes <out_prefix>.blocks.tsv, .block_calls.tsv and .block_donors.tsv; returns a
    dict with the engine's arrays, the statistics, the donor table and the flag counts."""
    from . import capi, engine
    mode = capi.DMX_MODE_STRICT if mode is None else mode
    g = np.ascontiguousarray(g, dtype=np.float32)
    if int(min_blocks) < 0 or int(min_cells) < 0:
        raise ValueError("min_blocks and min_cells must not be negative")
    if isinstance(store_or_pileup, engine.HostPileup):
        pl = store_or_pileup
        if barcodes is None:
            raise ValueError("block_run: a HostPileup needs barcodes=")
    else:
        pl, barcodes = store_or_pileup.freeze(), store_or_pileup.barcodes()
    if g.ndim != 3 or g.shape[0] != pl.n_snps or g.shape[1] != len(sample_ids) or g.shape[2] != 3:
        raise ValueError(f"genotype matrix {g.shape} for {pl.n_snps} SNPs and {len(sample_ids)} samples")
    if snps is None:
        snps = [(0, i, ".", ".") for i in range(pl.n_snps)]
    if len(snps) != pl.n_snps:
        raise ValueError(f"snps: {len(snps)} rows for {pl.n_snps} SNPs")
    ids, table = block if block is not None else make_blocks(snps, n_blocks, block_bp, by_chrom)
    G = int(ids.max()) + 1 if len(ids) else 1
    if best is None:
        engine.demuxlet_run(pl, g, sample_ids, alphas, out_prefix, barcodes=barcodes, device=device, mode=mode, **demuxlet_run_kwargs)
        best = out_prefix + ".best"
    rows = read_best_rows(best, sample_ids, barcodes, alphas)
    eng = engine.Engine(len(sample_ids), alphas, device=device, mode=mode)
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        res = eng.block_llk(ids, G, extras_from_rows(rows))
        info = eng.block_llk_info()
    finally:
        eng.close()
    st = block_calls(res, rows, min_blocks)
    donors = block_donors(res, rows, min_cells)
    write_blocks_tsv(out_prefix + ".blocks.tsv", table)
    flags = write_calls_tsv(out_prefix + ".block_calls.tsv", barcodes, sample_ids, alphas, rows, st)
    n_swap = write_donors_tsv(out_prefix + ".block_donors.tsv", sample_ids, donors)
    return dict(block=ids, table=table, res=res, info=info, rows=rows, calls=st, donors=donors, flags=flags, n_swap=n_swap, best=best)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.blocks",
                                 description="block-resolved likelihoods: jackknife errors and leave-one-block-out calls")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.blocks.tsv, .block_calls.tsv, .block_donors.tsv (and <out>.best/... without --best)")
    ap.add_argument("--best", help="a .best of this pileup (default: run the demultiplexing pass first)")
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--blocks", type=int, default=None, help="about this many blocks of equal SNP count, shared out by chromosome (default 40)")
    how.add_argument("--block-bp", type=int, default=None, help="windows of this many bases instead")
    how.add_argument("--by-chrom", action="store_true", help="one block per chromosome instead")
    ap.add_argument("--min-blocks", type=int, default=5, help="FLAG is LOWN below this many covered blocks (default 5)")
    ap.add_argument("--min-cells", type=int, default=10, help="a donor row is SWAP? only with at least this many cells (default 10)")
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.0, 0.5], help="doublet grid of the demultiplexing pass (default 0 0.5)")
    ap.add_argument("--fast", action="store_true", help="DMX_MODE_FAST for the demultiplexing pass (the block sums are STRICT terms either way)")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    if a.blocks is not None and a.blocks < 1:
        ap.error("--blocks must be at least 1")
    if a.block_bp is not None and a.block_bp < 1:
        ap.error("--block-bp must be at least 1")
    if a.min_blocks < 0 or a.min_cells < 0:
        ap.error("--min-blocks and --min-cells must not be negative")
    if a.blocks is None and a.block_bp is None and not a.by_chrom:
        a.blocks = 40
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    from . import capi, refine
    d = refine.read_pileup_txt(a.pileup)
    r = block_run(d.pileup, d.g, d.sample_ids, a.out, snps=d.snps, best=a.best, n_blocks=a.blocks, block_bp=a.block_bp, by_chrom=a.by_chrom,
                  min_blocks=a.min_blocks, min_cells=a.min_cells, alphas=a.alpha, barcodes=d.barcodes, device=a.gpu,
                  mode=capi.DMX_MODE_FAST if a.fast else capi.DMX_MODE_STRICT)
    f = r["flags"]
    print(f"{len(r['table'])} blocks; {f['STABLE']} barcodes STABLE, {f['FRAGILE']} FRAGILE, {f['LOWN']} LOWN; {r['n_swap']} donor rows SWAP?",
          file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
