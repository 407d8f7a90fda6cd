"""Donor relatedness, separability and cross-run matching from joint genotype tables.

Every other pass compares reads with genotype columns.  This one compares genotype columns with each other: Engine.geno_compare
(dmx_engine_geno_compare) gives, for every pair (a, b) of columns of two gp-style matrices, the weighted 4 x 4 table
T[x][y] = sum_i c_i ra_i[x] rb_i[y] with r = (p0, p1, p2, valid).  J = T[0..2][0..2] is the joint genotype table under independent draws
from the two rows and N = T[3][3] the weight of the jointly valid SNPs.  From them:

    IBS0 = (J02 + J20) / N,  IBS2 = trace J / N,  DISC = 1 - IBS2,  R.DOSAGE = the Pearson correlation of the dosages,
    KIN  = (J11 - 2 (J02 + J20)) / (sum_y J[1][y] + sum_x J[x][1])                 (KING-robust)
    LLR.AB = sum_xy Jc_ab[x][y] KL[x][y]     the expected log-likelihood ratio by which a cell of donor a prefers a over b, with Jc the
             table weighted by c_i = stored reads at SNP i / barcodes with a stored read, and KL the per-read table of kl_table().

    python -m demuxlet_amd.kin --pileup <x>.pileup.txt --out <prefix> [--genotypes <x>.clust.tsv|<x>.refined.tsv]
        [--against <y>.pileup.txt | <y>.clust.tsv | <y>.refined.tsv] [--margin 2] [--min-snp 100] [--gpu G]

Without --against (audit): the matrix against itself -> <prefix>.kin.tsv (one row per unordered pair) and <prefix>.kin_donors.tsv.
With --against (match): A = the dump's matrix or --genotypes, B = the other file's matrix, SNPs aligned on (RID, POS, REF, ALT)
-> <prefix>.kin_match.tsv with the one-to-one assignment that maximises the sum of KIN.

Limits: the statistics are expectations under independent draws from the two rows, so soft rows shrink KIN and raise DISC even for
identical donors; KING's bands are for hard calls without strong population structure; LLR is a mean at the pool's mean depth and
overstates what the singlet pass sees where (barcode, SNP) pairs hold several reads (that pass floors a pair's likelihoods once);
swapped REF / ALT between files is dropped, not repaired."""
from __future__ import annotations

import argparse
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import engine, refine

KIN_DUP, KIN_REL1, KIN_REL2 = 0.354, 0.177, 0.0884      # KING's inference bands for hard calls
PAIR_HEADER = "SM_A\tSM_B\tN.SNP\tIBS0\tIBS2\tDISC\tR.DOSAGE\tKIN\tLLR.AB\tLLR.BA\tFLAG\n"
DONOR_HEADER = "SM_ID\tN.VALID\tHET\tNEAREST\tKIN\tLLR\n"
MATCH_HEADER = "SM_A\tBEST_B\tKIN\tDISC\tN.SNP\tSECOND_B\tKIN.2ND\tASSIGN\n"
Key = Tuple[str, int, str, str]


# ---------------------------------------------------------------------------------------------------------------------
# statistics of a table [..][4][4]

def pair_stats(T: np.ndarray) -> Dict[str, np.ndarray]:
    """N, IBS0, IBS2, DISC, R (dosage correlation) and KIN of every table in T[..., 4, 4]; nan where a denominator is zero."""
    T = np.asarray(T, dtype=np.float64)
    J = T[..., :3, :3]
    N = T[..., 3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        ibs0 = (J[..., 0, 2] + J[..., 2, 0]) / N
        ibs2 = (J[..., 0, 0] + J[..., 1, 1] + J[..., 2, 2]) / N
        ra, rb = J.sum(axis=-1), J.sum(axis=-2)                 # the marginals of a and of b over the jointly valid SNPs
        tot = ra.sum(axis=-1)
        d = np.arange(3.0)
        ea, eb = (ra * d).sum(-1) / tot, (rb * d).sum(-1) / tot
        va, vb = (ra * d * d).sum(-1) / tot - ea * ea, (rb * d * d).sum(-1) / tot - eb * eb
        eab = (J * np.outer(d, d)).sum(axis=(-1, -2)) / tot
        r = (eab - ea * eb) / np.sqrt(va * vb)
        het = ra[..., 1] + rb[..., 1]
        kin = np.where(het > 0, (J[..., 1, 1] - 2.0 * (J[..., 0, 2] + J[..., 2, 0])) / het, np.nan)     # undefined without a heterozygote
    return {"N": N, "IBS0": ibs0, "IBS2": ibs2, "DISC": 1.0 - ibs2, "R": r, "KIN": kin}


def llr(Tc: np.ndarray, kl: np.ndarray) -> np.ndarray:
    """sum_xy Tc[..][x][y] KL[x][y] over the genotype block of weighted tables."""
    return (np.asarray(Tc)[..., :3, :3] * kl).sum(axis=(-1, -2))


GL_FLOOR = 1e-6     # the singlet pass adds this to a pair's normalised genotype likelihoods (cmd_cram_demuxlet.cpp:446-452)


def read_probs(mat: np.ndarray, err: np.ndarray):
    """By base quality q < 128: L[q][g][al], the singlet pass's likelihood of a read with allele al under genotype g (pR, (pR + pA) / 2,
    pA with pR / pA = mat or err / 3), and P[q][g][al], the law of a stored read's allele under genotype g (L normalised over al)."""
    m, e3 = np.asarray(mat, dtype=np.float64)[:128], np.asarray(err, dtype=np.float64)[:128] / 3.0
    L = np.zeros((128, 3, 2))
    L[:, 0, 0] = m; L[:, 0, 1] = e3
    L[:, 2, 0] = e3; L[:, 2, 1] = m
    L[:, 1, :] = ((m + e3) * 0.5)[:, None]
    return L, L / L.sum(axis=2, keepdims=True)


def kl_table(mat: np.ndarray, err: np.ndarray, bq_hist: np.ndarray) -> np.ndarray:
    """KL[x][y] = E[log GL_x - log GL_y] for one read drawn under genotype x, averaged over the base qualities with the weights
    bq_hist[128] (counts of stored reads).  GL is what the singlet pass takes the log of for a hard row: the read's likelihoods
    normalised over the three genotypes, plus GL_FLOOR, normalised again; the floor keeps every entry finite."""
    L, P = read_probs(mat, err)
    w = np.asarray(bq_hist, dtype=np.float64)[:128]
    if not w.sum() > 0:
        return np.zeros((3, 3))
    w = w / w.sum()
    gl = L / L.sum(axis=1, keepdims=True) + GL_FLOOR
    lg = np.log(gl / gl.sum(axis=1, keepdims=True))                 # [q][g][al]
    kl = np.zeros((3, 3))
    for x in range(3):
        for y in range(3):
            kl[x, y] = (w[:, None] * P[:, x, :] * (lg[:, x, :] - lg[:, y, :])).sum()
    return kl


def pool_weight(pl: engine.HostPileup):
    """(c[S], bq_hist[128], n_barcodes): c_i = stored reads at SNP i / barcodes with at least one stored read."""
    B, S = pl.n_cells, pl.n_snps
    nrd = np.asarray(pl.pair_nrd).astype(np.int64)
    if pl.pair_snp is not None:
        snp = np.asarray(pl.pair_snp).astype(np.int64)
    else:
        snp = np.arange(len(nrd), dtype=np.int64) - np.repeat(np.asarray(pl.cell_pair_off[:-1], dtype=np.int64), np.diff(pl.cell_pair_off))
    per_snp = np.bincount(snp, weights=nrd, minlength=S)[:S] if len(nrd) else np.zeros(S)
    n_bc = int((np.diff(np.asarray(pl.cell_read_off, dtype=np.int64)) > 0).sum()) if B else 0
    hist = np.bincount(np.asarray(pl.reads, dtype=np.uint8) & 127, minlength=128).astype(np.float64)
    return (per_snp / n_bc if n_bc else np.zeros(S)), hist, n_bc


def flag_of(n: float, kin: float, llr_min: Optional[float], margin: float, min_snp: int) -> str:
    if not n >= min_snp:
        return "LOWN"
    f = []
    if kin > KIN_DUP: f.append("DUP")
    elif kin > KIN_REL1: f.append("REL1")
    elif kin > KIN_REL2: f.append("REL2")
    if llr_min is not None and llr_min < margin: f.append("INSEP")
    return ",".join(f) if f else "."


# ---------------------------------------------------------------------------------------------------------------------
# one-to-one assignment

def assign_max(gain: np.ndarray, allowed: Optional[np.ndarray] = None) -> np.ndarray:
    """out[i] = the column given to row i, or -1: the one-to-one partial assignment that maximises the sum of gain over its pairs.  Only
    allowed pairs with gain > 0 are ever chosen (an unassigned row counts 0), so a rectangular or masked table leaves the surplus
    unassigned.  Hungarian algorithm with potentials over a cost matrix padded with one zero-cost dummy column per row."""
    gain = np.asarray(gain, dtype=np.float64)
    nA, nB = gain.shape
    ok = np.isfinite(gain) & (gain > 0)
    if allowed is not None:
        ok &= np.asarray(allowed, dtype=bool)
    g = np.where(ok, gain, 0.0)
    out = np.full(nA, -1, dtype=np.int64)
    if nA == 0:
        return out
    m = nB + nA
    cost = np.zeros((nA, m)); cost[:, :nB] = -g
    u = np.zeros(nA + 1); v = np.zeros(m + 1)
    p = np.zeros(m + 1, dtype=np.int64); way = np.zeros(m + 1, dtype=np.int64)
    for i in range(1, nA + 1):
        p[0] = i; j0 = 0
        minv = np.full(m + 1, np.inf); used = np.zeros(m + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            free = ~used[1:]
            upd = free & (cur < minv[1:])
            minv[1:][upd] = cur[upd]; way[1:][upd] = j0
            cand = np.where(free, minv[1:], np.inf)
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[p[used]] += delta; v[used] -= delta            # (the used columns hold distinct rows)
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]; p[j0] = p[j1]; j0 = j1
    for j in range(1, nB + 1):
        if p[j] and ok[p[j] - 1, j - 1]:
            out[p[j] - 1] = j - 1
    return out


# ---------------------------------------------------------------------------------------------------------------------
# readers and alignment

def snp_keys(snps: Sequence[Tuple]) -> List[Key]:
    return [(str(r), int(p), str(a), str(b)) for r, p, a, b in snps]


def read_genotype_tsv(path: str):
    """A .clust.tsv / .refined.tsv (refine.write_refined_tsv's format; covered rows only) as (keys, sample_ids, rows): the SNP keys and
    the samples in order of first appearance, rows = {(snp index, sample index): (gp0, gp1, gp2)}."""
    keys: List[Key] = []; kidx: Dict[Key, int] = {}
    ids: List[str] = []; sidx: Dict[str, int] = {}
    rows: Dict[Tuple[int, int], Tuple[float, float, float]] = {}
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        col = {n: i for i, n in enumerate(head)}
        for n in ("RID", "POS", "REF", "ALT", "SM_ID", "GP0", "GP1", "GP2"):
            if n not in col:
                raise ValueError(f"{path}: no {n} column")
        for ln, line in enumerate(f, 2):
            t = line.rstrip("\n").split("\t")
            if len(t) == 1 and not t[0]:
                continue
            if len(t) < len(head):
                raise ValueError(f"{path}:{ln}: {len(t)} fields, the header has {len(head)}")
            k = (t[col["RID"]], int(t[col["POS"]]), t[col["REF"]], t[col["ALT"]])
            i = kidx.setdefault(k, len(keys))
            if i == len(keys): keys.append(k)
            j = sidx.setdefault(t[col["SM_ID"]], len(ids))
            if j == len(ids): ids.append(t[col["SM_ID"]])
            rows[(i, j)] = (float(t[col["GP0"]]), float(t[col["GP1"]]), float(t[col["GP2"]]))
    return keys, ids, rows


def matrix_of_rows(n_snps: int, n_samples: int, rows) -> np.ndarray:
    """float32 [n_snps][n_samples][3]; a (SNP, sample) that `rows` does not list stays all zero (an invalid row)."""
    g = np.zeros((n_snps, n_samples, 3), dtype=np.float32)
    for (i, j), r in rows.items():
        g[i, j] = r
    return g


def load_matrix(path: str):
    """(keys, sample_ids, g) of a .pileup.txt dump or a genotype tsv."""
    if path.endswith(".pileup.txt"):
        d = refine.read_pileup_txt(path)
        return snp_keys(d.snps), list(d.sample_ids), d.g
    keys, ids, rows = read_genotype_tsv(path)
    return keys, ids, matrix_of_rows(len(keys), len(ids), rows)


def onto_keys(keys_to: Sequence[Key], keys: Sequence[Key], g: np.ndarray):
    """g's rows placed on another SNP list: (matrix over keys_to, records of g that keys_to does not have)."""
    at = {k: i for i, k in enumerate(keys_to)}
    out = np.zeros((len(keys_to),) + g.shape[1:], dtype=np.float32)
    miss = 0
    for i, k in enumerate(keys):
        j = at.get(k)
        if j is None: miss += 1
        else: out[j] = g[i]
    return out, miss


def align(keys_a: Sequence[Key], ga: np.ndarray, keys_b: Sequence[Key], gb: np.ndarray):
    """Both matrices over one SNP list: A's records in order, then the records only B has.  A record that one side lacks is an all-zero
    (invalid) row there.  A position (RID, POS) where a record of one file has no exact partner although the other file has a record at
    that position (its REF / ALT differ, swapped for instance) is dropped on both sides and counted.
    Returns (keys, ga', gb', dict(shared, only_a, only_b, allele_mismatch))."""
    sa, sb = set(keys_a), set(keys_b)
    pa, pb = {k[:2] for k in keys_a}, {k[:2] for k in keys_b}
    bad = {k[:2] for k in sa - sb if k[:2] in pb} | {k[:2] for k in sb - sa if k[:2] in pa}
    keys = [k for k in keys_a if k[:2] not in bad] + [k for k in keys_b if k not in sa and k[:2] not in bad]
    ga2, _ = onto_keys(keys, keys_a, ga)
    gb2, _ = onto_keys(keys, keys_b, gb)
    kept = set(keys)
    info = dict(shared=len(kept & sa & sb), only_a=len((kept & sa) - sb), only_b=len((kept & sb) - sa), allele_mismatch=len(bad))
    return keys, ga2, gb2, info


# ---------------------------------------------------------------------------------------------------------------------
# the two modes

def _fmt(x: float) -> str:
    return "nan" if not np.isfinite(x) else f"{x:.6g}"


def kin_run(ga: np.ndarray, ids_a: Sequence[str], out_prefix: str, gb: Optional[np.ndarray] = None, ids_b: Optional[Sequence[str]] = None,
            pileup: Optional[engine.HostPileup] = None, weight: Optional[np.ndarray] = None, kl: Optional[np.ndarray] = None,
            margin: float = 2.0, min_snp: int = 100, device: int = 0) -> dict:
    """gb = None (audit): ga against itself -> <out_prefix>.kin.tsv and .kin_donors.tsv.  The LLR columns need the pool: `pileup` (the
    weight and KL are taken from it and the engine's phred tables) or `weight` [S] with `kl` [3][3]; without either they are nan and
    INSEP is not given.  gb given (match): -> <out_prefix>.kin_match.tsv.  Returns the arrays behind the files."""
    ga = np.ascontiguousarray(ga, dtype=np.float32)
    VA = ga.shape[1]
    if len(ids_a) != VA:
        raise ValueError(f"{len(ids_a)} sample ids for {VA} columns")
    eng = engine.Engine(VA, device=device)
    try:
        if gb is None:
            T, nva, _ = eng.geno_compare(ga)
            info = eng.geno_compare_info()
            st = pair_stats(T)
            Tc = None
            if pileup is not None:
                if pileup.n_snps != ga.shape[0]:
                    raise ValueError(f"the pileup has {pileup.n_snps} SNPs, the matrix {ga.shape[0]}")
                weight, hist, _ = pool_weight(pileup)
                kl = kl_table(*engine.phred_tables(), hist)
            if weight is not None:
                if kl is None:
                    raise ValueError("weight needs kl")
                Tc, _, _ = eng.geno_compare(ga, weight=weight)
                info_w = eng.geno_compare_info()
                info = dict(info, rows_ms=info["rows_ms"] + info_w["rows_ms"], tile_ms=info["tile_ms"] + info_w["tile_ms"])
            L = llr(Tc, kl) if Tc is not None else np.full((VA, VA), np.nan)
            flags = {}
            with open(out_prefix + ".kin.tsv", "w") as f:
                f.write(PAIR_HEADER)
                for a in range(VA):
                    for b in range(a + 1, VA):
                        lm = min(L[a, b], L[b, a]) if Tc is not None else None
                        fl = flag_of(st["N"][a, b], st["KIN"][a, b], lm, margin, min_snp)
                        flags[(a, b)] = fl
                        f.write(f"{ids_a[a]}\t{ids_a[b]}\t{int(round(st['N'][a, b]))}\t{_fmt(st['IBS0'][a, b])}\t{_fmt(st['IBS2'][a, b])}\t"
                                f"{_fmt(st['DISC'][a, b])}\t{_fmt(st['R'][a, b])}\t{_fmt(st['KIN'][a, b])}\t{_fmt(L[a, b])}\t{_fmt(L[b, a])}\t{fl}\n")
            kin_m = np.where((st["N"] >= min_snp) & np.isfinite(st["KIN"]), st["KIN"], -np.inf)
            np.fill_diagonal(kin_m, -np.inf)
            with open(out_prefix + ".kin_donors.tsv", "w") as f:
                f.write(DONOR_HEADER)
                for a in range(VA):
                    n_self = T[a, a, 3, 3]
                    het = T[a, a, 1, 3] / n_self if n_self > 0 else np.nan
                    b = int(np.argmax(kin_m[a])) if VA > 1 and np.isfinite(kin_m[a].max()) else -1
                    f.write(f"{ids_a[a]}\t{int(nva[a])}\t{_fmt(het)}\t{ids_a[b] if b >= 0 else '.'}\t{_fmt(st['KIN'][a, b]) if b >= 0 else 'nan'}\t"
                            f"{_fmt(L[a, b]) if b >= 0 else 'nan'}\n")
            return dict(table=T, table_weighted=Tc, stats=st, llr=L, flags=flags, n_valid=nva, info=info, weight=weight, kl=kl)
        gb = np.ascontiguousarray(gb, dtype=np.float32)
        VB = gb.shape[1]
        if ids_b is None or len(ids_b) != VB:
            raise ValueError(f"match mode needs {VB} sample ids for B")
        if gb.shape[0] != ga.shape[0]:
            raise ValueError(f"A has {ga.shape[0]} SNPs, B has {gb.shape[0]} (align them first)")
        T, nva, nvb = eng.geno_compare(ga, gb)
        info = eng.geno_compare_info()
        st = pair_stats(T)
        ok = (st["N"] >= min_snp) & np.isfinite(st["KIN"])
        asg = assign_max(np.where(ok, st["KIN"], 0.0), ok)
        kin_m = np.where(ok, st["KIN"], -np.inf)
        with open(out_prefix + ".kin_match.tsv", "w") as f:
            f.write(MATCH_HEADER)
            for a in range(VA):
                order = np.argsort(-kin_m[a], kind="stable")
                b1 = int(order[0]) if np.isfinite(kin_m[a, order[0]]) else -1
                b2 = int(order[1]) if VB > 1 and np.isfinite(kin_m[a, order[1]]) else -1
                f.write(f"{ids_a[a]}\t{ids_b[b1] if b1 >= 0 else '.'}\t{_fmt(st['KIN'][a, b1]) if b1 >= 0 else 'nan'}\t"
                        f"{_fmt(st['DISC'][a, b1]) if b1 >= 0 else 'nan'}\t{int(round(st['N'][a, b1])) if b1 >= 0 else 0}\t"
                        f"{ids_b[b2] if b2 >= 0 else '.'}\t{_fmt(st['KIN'][a, b2]) if b2 >= 0 else 'nan'}\t{ids_b[asg[a]] if asg[a] >= 0 else '.'}\n")
        return dict(table=T, stats=st, assign=asg, n_valid_a=nva, n_valid_b=nvb, info=info)
    finally:
        eng.close()


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.kin", description="donor relatedness, separability and cross-run matching from joint genotype tables")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.kin.tsv and <out>.kin_donors.tsv, or <out>.kin_match.tsv with --against")
    ap.add_argument("--genotypes", help="a .clust.tsv / .refined.tsv whose matrix replaces the dump's")
    ap.add_argument("--against", help="match mode: a .pileup.txt, .clust.tsv or .refined.tsv to match the columns against")
    ap.add_argument("--margin", type=float, default=2.0, help="INSEP below this expected log-likelihood ratio (default 2)")
    ap.add_argument("--min-snp", type=int, default=100, help="LOWN below this many jointly valid SNPs (default 100)")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    if not a.margin >= 0.0:
        ap.error("--margin must be >= 0")
    if a.min_snp < 0:
        ap.error("--min-snp must be >= 0")
    try:
        d = refine.read_pileup_txt(a.pileup)
        keys, ids, g = snp_keys(d.snps), list(d.sample_ids), d.g
        if a.genotypes:
            k2, ids, g2 = load_matrix(a.genotypes)
            g, miss = onto_keys(keys, k2, g2)
            if miss:
                print(f"kin: {miss} SNP records of {a.genotypes} are not in the dump and were dropped", file=sys.stderr)
        if len(ids) < 1:
            raise ValueError("no genotype columns")
        if a.against:
            kb, ids_b, gb = load_matrix(a.against)
            if len(ids_b) < 1:
                raise ValueError(f"{a.against}: no genotype columns")
            _, ga2, gb2, inf = align(keys, g, kb, gb)
            print(f"kin: {inf['shared']} shared SNPs, {inf['only_a']} only in A, {inf['only_b']} only in B, "
                  f"{inf['allele_mismatch']} positions with different REF/ALT dropped", file=sys.stderr)
            kin_run(ga2, ids, a.out, gb=gb2, ids_b=ids_b, min_snp=a.min_snp, device=a.gpu)
        else:
            kin_run(g, ids, a.out, pileup=d.pileup, margin=a.margin, min_snp=a.min_snp, device=a.gpu)
    except (OSError, ValueError) as ex:
        print(f"kin: {ex}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
