"""The reference of the CPU tests of demuxlet_amd/blocks.py (test infrastructure: never imported by the product, never read by a GPU test).

Per-block values: the oracle's llksAB / llks00 on each block's sub-pileup — what the kernel's contract says block g's values are.
Statistics: the jackknife, the leave-one-block-out rule and the donor table restated in straight loops over Python floats, in the
operation order the module's docstring gives."""
import math

import numpy as np

import quality_mix as Q

SNG, DBL, AMB = 0, 1, 2


def sub_pileup(engine, pl, keep_snp):
    """The pileup with only the pairs at the SNPs of keep_snp[S] (bool)."""
    po = np.asarray(pl.cell_pair_off, dtype=np.int64)
    nrd = np.asarray(pl.pair_nrd).astype(np.int64)
    cell = np.repeat(np.arange(pl.n_cells), np.diff(po))
    snp = np.asarray(pl.pair_snp, dtype=np.int32)
    keep = np.asarray(keep_snp, dtype=bool)[snp]
    new_po = np.concatenate([[0], np.cumsum(np.bincount(cell[keep], minlength=pl.n_cells))]).astype(np.int64)
    new_ro = np.concatenate([[0], np.cumsum(np.bincount(cell[keep], weights=nrd[keep], minlength=pl.n_cells))]).astype(np.int64)
    reads = np.asarray(pl.reads, dtype=np.uint8)[np.repeat(keep, nrd)]
    return engine.HostPileup(pl.n_cells, pl.n_snps, new_po, new_ro, np.ascontiguousarray(snp[keep]), np.ascontiguousarray(np.asarray(pl.pair_nrd)[keep]),
                             np.ascontiguousarray(reads), pl.rd_totl, pl.rd_pass, pl.rd_uniq)


def oracle_grid(oracle, pl, g, alphas):
    r = Q.oracle_run(oracle, pl, g, alphas)
    return r.llksAB.reshape(pl.n_cells, g.shape[1], g.shape[1], len(alphas)), r.llks00.reshape(pl.n_cells, len(alphas))


def block_values(oracle, engine, pl, g, alphas, block, G, extra):
    """col[B][G][V], l00[B][G][A], ext[B][G][E], n_snp[B][G] from one oracle run per occupied block."""
    B, V, A, E = pl.n_cells, g.shape[1], len(alphas), extra.shape[1]
    col, l00, ext = np.zeros((B, G, V)), np.zeros((B, G, A)), np.zeros((B, G, E))
    n_snp = np.zeros((B, G), dtype=np.int32)
    for gid in sorted(set(int(x) for x in block)):
        sub = sub_pileup(engine, pl, block == gid)
        grid, z = oracle_grid(oracle, sub, g, alphas)
        col[:, gid], l00[:, gid], n_snp[:, gid] = grid[:, :, 0, 0], z, np.diff(sub.cell_pair_off)
        for b in range(B):
            for s in range(E):
                j, k, n = extra[b, s]
                if j >= 0:
                    ext[b, gid, s] = grid[b, j, k, n]
    return dict(col=col, l00=l00, ext=ext, n_snp=n_snp)


def scan_singlets(col):
    """cmd_cram_demuxlet.cpp:746-758 on one barcode's singlet column."""
    i1 = i2 = -1
    m1 = m2 = -1e300
    for j, x in enumerate(col):
        if m1 < x:
            m2, i2, i1, m1 = m1, i1, j, x
        elif m2 < x:
            i2, m2 = j, x
    return i1, i2


def scan_doublet(grid):
    """:799-814 on one barcode's grid [V][V][A]."""
    V, _, A = grid.shape
    jb = kb = nb = -1
    mx = -1e300
    for j in range(V):
        for k in range(V):
            if j == k:
                continue
            for n in range(1, A):
                if mx < grid[j, k, n]:
                    jb, kb, nb, mx = j, k, n, grid[j, k, n]
    return jb, kb, nb


def rule(col, llk12, jb, kb):
    """:816-857: (kind, iSing1, iSing2)."""
    i1, i2 = scan_singlets(col)
    if llk12 > col[jb] and llk12 > col[kb] and llk12 > col[i1] + 2:
        return DBL, i1, i2
    if col[i1] > col[i2] + 2:
        return SNG, i1, i2
    return AMB, i1, i2


def rule_margins(col, llk12, jb, kb):
    """The distances from their thresholds of the comparisons that decide the call: for a doublet the smallest of its three; otherwise
    the clearest of the comparisons that reject the doublet, and the one between SNG and AMB."""
    i1, i2 = scan_singlets(col)
    d = [llk12 - col[jb], llk12 - col[kb], llk12 - (col[i1] + 2)]
    if min(d) > 0:
        return [min(d)]
    return [max(-x for x in d if x <= 0), abs(col[i1] - (col[i2] + 2))]


def best_rows(grid, sample_ids, alphas):
    """blocks.BestRows-like arrays from whole-genome grids [B][V][V][A] by the reference's scans and rule."""
    B = grid.shape[0]
    out = dict(best=[], kind=np.zeros(B, dtype=np.int8), sng1=np.zeros(B, dtype=np.int32), sng2=np.zeros(B, dtype=np.int32),
               dbl1=np.zeros(B, dtype=np.int32), dbl2=np.zeros(B, dtype=np.int32), n_alpha=np.zeros(B, dtype=np.int32))
    for b in range(B):
        jb, kb, nb = scan_doublet(grid[b])
        col = grid[b, :, 0, 0]
        kind, i1, i2 = rule(col, grid[b, jb, kb, nb], jb, kb)
        out["kind"][b], out["sng1"][b], out["sng2"][b], out["dbl1"][b], out["dbl2"][b], out["n_alpha"][b] = kind, i1, i2, jb, kb, nb
        sm = sample_ids
        out["best"].append(f"DBL-{sm[jb]}-{sm[kb]}-{alphas[nb]:.3f}" if kind == DBL else f"SNG-{sm[i1]}" if kind == SNG else
                           f"AMB-{sm[i1]}-{sm[i2]}-{sm[jb]}/{sm[kb]}")
    return out


def pick_order(e_ab, e_ba, d1, d2):
    """The order of the fixed pair the scan of :799-814 keeps: 0 = (d1, d2), 1 = (d2, d1)."""
    first = 0 if d1 <= d2 else 1
    ef, es = (e_ab, e_ba) if first == 0 else (e_ba, e_ab)
    return 1 - first if es > ef else first


def jackknife(d):
    """(D, SE) of the covered blocks' values d (a list): the delete-one jackknife of a total."""
    m = len(d)
    D = 0.0
    for x in d:
        D += x
    if m < 2:
        return D, math.nan
    mean = D / m
    ss = 0.0
    for x in d:
        ss += (x - mean) * (x - mean)
    return D, math.sqrt(m / (m - 1.0) * ss)


def calls_of(res, rows, b, min_blocks=5):
    """One barcode's statistics in straight loops: dict(m, llr_sng, se_sng, llr_dbl, se_dbl, top_block, top_share, loo_min, n_loo_same,
    loo (per covered block: (g, kind, s1, s2, order)), flag)."""
    col, ext, n_snp = res["col"][b], res["ext"][b], res["n_snp"][b]
    G, V = col.shape
    cov = [g for g in range(G) if n_snp[g] > 0]
    s1, s2, d1, d2, kind0 = int(rows["sng1"][b]), int(rows["sng2"][b]), int(rows["dbl1"][b]), int(rows["dbl2"][b]), int(rows["kind"][b])
    t_col = [0.0] * V
    t_ext = [0.0, 0.0]
    for g in range(G):
        for v in range(V):
            t_col[v] += float(col[g, v])
        for s in range(2):
            t_ext[s] += float(ext[g, s])
    o = pick_order(t_ext[0], t_ext[1], d1, d2)
    d_sng = [float(col[g, s1]) - float(col[g, s2]) for g in cov]
    d_dbl = [float(ext[g, o]) - float(col[g, s1]) for g in cov]
    D_s, se_s = jackknife(d_sng)
    D_d, se_d = jackknife(d_dbl)
    dec, D = (d_dbl, D_d) if kind0 == DBL else (d_sng, D_s)
    top = loo_min = None
    for i, g in enumerate(cov):
        if top is None or dec[i] > dec[top]:
            top = i
        if loo_min is None or D - dec[i] < loo_min:
            loo_min = D - dec[i]
    loo, n_same = [], 0
    for g in cov:
        c = [t_col[v] - float(col[g, v]) for v in range(V)]
        e = [t_ext[s] - float(ext[g, s]) for s in range(2)]
        ro = pick_order(e[0], e[1], d1, d2)
        jb, kb = (d1, d2) if ro == 0 else (d2, d1)
        kind, r1, r2 = rule(c, e[ro], jb, kb)
        same = kind == kind0 and (kind == DBL or r1 == s1) and (kind != AMB or r2 == s2)
        n_same += same
        loo.append((g, kind, r1, r2, ro, same))
    fragile = any(not x[5] for x in loo)
    flag = "LOWN" if len(cov) < min_blocks else "FRAGILE" if fragile else "STABLE"
    return dict(m=len(cov), llr_sng=D_s, se_sng=se_s, llr_dbl=D_d, se_dbl=se_d, top_block=cov[top] if cov else -1,
                top_share=dec[top] / D if cov else math.nan, loo_min=loo_min if cov else math.nan, n_loo_same=n_same, loo=loo, flag=flag, order=o)


def donors_of(res, rows, min_cells=10):
    """The donor table in straight loops: the rows of blocks.block_donors."""
    col, n_snp = res["col"], res["n_snp"]
    B, G, V = col.shape
    out = []
    for d in range(V):
        for g in range(G):
            n_cell = n_s = n_other = 0
            llr = 0.0
            votes = [0] * V
            for b in range(B):
                if rows["kind"][b] != SNG or rows["sng1"][b] != d or n_snp[b, g] <= 0:
                    continue
                n_cell += 1
                n_s += int(n_snp[b, g])
                llr += float(col[b, g, d]) - float(col[b, g, rows["sng2"][b]])
                top = 0
                for v in range(1, V):
                    if col[b, g, v] > col[b, g, top]:
                        top = v
                if top != d:
                    n_other += 1
                    votes[top] += 1
            if n_cell:
                bo = max(range(V), key=lambda v: (votes[v], -v)) if n_other else -1
                out.append((d, g, n_cell, n_s, llr, n_other, bo, "SWAP?" if n_cell >= min_cells and 2 * n_other > n_cell else "."))
    return out
