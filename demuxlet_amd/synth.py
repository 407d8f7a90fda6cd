"""Synthetic pileups for the BASELINE.json configs.

Generative model (ours; the reference ships no generator): per SNP AF ~ U(0.05,0.95), per-sample genotype ~
Binomial(2, AF); a cell is a singlet of sample (c mod V) w.p. 0.9, else a 50/50 doublet with a second, different
sample; each (cell, SNP) is covered w.p. delta; a covered pair carries 1+Poisson(rbar-1) unique UMIs; a read shows ALT
w.p. g/2 of its source sample, bq ~ U{13..40} (or another quality profile, see draw_bq), and a base error w.p. 10^(-bq/10)
moves it to one of the three other bases (so allele 2 = "other" occurs).

Two back-ends:
  * numpy  (host; tests, fixtures, small problems, events with strings for the UMI-store path)
  * torch  (device; bench-scale problems are generated directly in HBM so nothing crosses PCIe)
The packed read byte is the C-ABI's: (allele<<7)|bq with allele in {0,1}; allele-2 reads are dropped from the byte
stream (they are skipped by both likelihood loops, cmd_cram_demuxlet.cpp:435,:604) but still create the pair.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np


@dataclass
class RawGeno:
    alleles: np.ndarray            # int32 [S][V][2]   (-1 = missing)
    af: np.ndarray                 # float64 [S]


def make_raw_genotypes(rng: np.random.Generator, S: int, V: int, missing_rate: float = 0.0) -> RawGeno:
    af = rng.uniform(0.05, 0.95, size=S)
    a = (rng.random((S, V, 2)) < af[:, None, None]).astype(np.int32)
    a.sort(axis=2)
    if missing_rate > 0:
        miss = rng.random((S, V)) < missing_rate
        a[miss] = -1
    return RawGeno(a, af)


def raw_gp_from_alleles(rng: np.random.Generator, alleles: np.ndarray, soft: float = 0.05) -> np.ndarray:
    """'softened one-hot' raw GP field (SURVEY §8d cfg 3): un-normalised floats, mostly on the true genotype."""
    S, V, _ = alleles.shape
    gt = np.clip(alleles, 0, 1).sum(axis=2)
    gp = rng.uniform(0.0, soft, size=(S, V, 3)).astype(np.float32)
    np.put_along_axis(gp, gt[..., None], (1.0 - rng.uniform(0, soft, size=(S, V, 1))).astype(np.float32), axis=2)
    return gp


def raw_pl_from_alleles(rng: np.random.Generator, alleles: np.ndarray) -> np.ndarray:
    """PL field (SURVEY §8d cfg 5): PL[true genotype]=0, others U{10..255}."""
    S, V, _ = alleles.shape
    gt = np.clip(alleles, 0, 1).sum(axis=2)
    pl = rng.integers(10, 256, size=(S, V, 3)).astype(np.int32)
    np.put_along_axis(pl, gt[..., None], 0, axis=2)
    return pl


# base qualities where the engine changes code path (pair / triple / LDS tables, PhredHelper's 0.75 floor at q <= 1, the top of the ABI)
EDGE_QUALS = np.array([0, 1, 2, 12, 13, 40, 41, 42, 47, 48, 63, 64, 93, 126, 127], dtype=np.uint8)
QUAL_PROFILES = (None, "full", "edges", "max")          # None (or "default"): U{13..40}
ERR_OF_BQ = np.power(10.0, -np.arange(128) / 10.0)


def draw_bq(rng: np.random.Generator, n: int, quals: Optional[str] = None) -> np.ndarray:
    """n base qualities of a profile: None = U{13..40} (the only draw of the default, so seeded problems do not change), "full" = U{0..127}
    (the whole C-ABI range), "edges" = half EDGE_QUALS, half U{13..40} (so pairs mix both), "max" = every read at 127 (no draw)."""
    if quals is None or quals == "default":
        return rng.integers(13, 41, size=n).astype(np.uint8)
    if quals == "full":
        return rng.integers(0, 128, size=n).astype(np.uint8)
    if quals == "edges":
        edge = EDGE_QUALS[rng.integers(0, len(EDGE_QUALS), size=n)]
        return np.where(rng.random(n) < 0.5, edge, rng.integers(13, 41, size=n)).astype(np.uint8)
    if quals == "max":
        return np.full(n, 127, dtype=np.uint8)
    raise ValueError(f"unknown quality profile {quals!r}")


@dataclass
class SynthPileup:
    """CSR pileup in the C-ABI's layout (cells in id order)."""
    n_cells: int
    n_snps: int
    cell_pair_off: np.ndarray      # int64 [B+1]
    cell_read_off: np.ndarray      # int64 [B+1]
    pair_snp: Optional[np.ndarray]  # int32 [P]  (None: dense, pair index within a cell == snp id)
    pair_nrd: np.ndarray           # uint8/uint16 [P]  reads kept per pair (allele 2 dropped)
    reads: np.ndarray              # uint8 [R]   (allele<<7)|bq
    rd_totl: np.ndarray            # int32 [B]
    rd_pass: np.ndarray
    rd_uniq: np.ndarray
    truth: np.ndarray              # int32 [B][2]  true (sample1, sample2 or -1)


def make_pileup(rng: np.random.Generator, alleles: np.ndarray, B: int, delta: float, rbar: float,
                dense_layout: bool = False, doublet_rate: float = 0.1, chunk_cells: int = 256, quals: Optional[str] = None) -> SynthPileup:
    """`quals`: the base-quality profile of the reads (draw_bq)."""
    S, V, _ = alleles.shape
    dosage = np.clip(alleles, 0, 1).sum(axis=2).astype(np.float64)      # [S][V]
    cell_pair_off = np.zeros(B + 1, dtype=np.int64)
    cell_read_off = np.zeros(B + 1, dtype=np.int64)
    snp_chunks, nrd_chunks, rd_chunks = [], [], []
    totl = np.zeros(B, dtype=np.int32)
    uniq = np.zeros(B, dtype=np.int32)
    truth = np.full((B, 2), -1, dtype=np.int32)
    for c0 in range(0, B, chunk_cells):
        c1 = min(B, c0 + chunk_cells)
        nc = c1 - c0
        s1 = (np.arange(c0, c1) % V).astype(np.int32)
        is_dbl = (rng.random(nc) < doublet_rate) & (V > 1)
        s2 = (s1 + 1 + rng.integers(0, max(V - 1, 1), size=nc)) % V
        truth[c0:c1, 0] = s1
        truth[c0:c1, 1] = np.where(is_dbl, s2, -1)
        if delta >= 1.0:
            cov = np.ones((nc, S), dtype=bool)
        else:
            cov = rng.random((nc, S)) < delta
        cc, ss = np.nonzero(cov)                                        # row-major: cell-major, snp ascending
        npairs = len(cc)
        nreads = 1 + rng.poisson(max(rbar - 1.0, 0.0), size=npairs)
        pair_of_read = np.repeat(np.arange(npairs), nreads)
        rc, rs = cc[pair_of_read], ss[pair_of_read]
        src = np.where(is_dbl[rc] & (rng.random(len(rc)) < 0.5), s2[rc], s1[rc])
        alt = rng.random(len(rc)) < dosage[rs, src] / 2.0
        bq = draw_bq(rng, len(rc), quals)
        e = rng.random(len(rc)) < ERR_OF_BQ[bq]
        u = rng.integers(0, 3, size=len(rc))
        allele = np.where(e, np.where(u == 0, 1 - alt.astype(np.int32), 2), alt.astype(np.int32)).astype(np.uint8)
        keep = allele != 2
        kept_per_pair = np.bincount(pair_of_read[keep], minlength=npairs)
        per_cell_pairs = np.bincount(cc, minlength=nc)
        per_cell_reads_all = np.bincount(rc, minlength=nc)
        per_cell_reads_kept = np.bincount(rc[keep], minlength=nc)
        cell_pair_off[c0 + 1:c1 + 1] = per_cell_pairs
        cell_read_off[c0 + 1:c1 + 1] = per_cell_reads_kept
        totl[c0:c1] = per_cell_reads_all
        uniq[c0:c1] = per_cell_reads_all
        snp_chunks.append(ss.astype(np.int32))
        nrd_chunks.append(kept_per_pair)
        rd_chunks.append(((allele[keep] << 7) | bq[keep]).astype(np.uint8))
    np.cumsum(cell_pair_off, out=cell_pair_off)
    np.cumsum(cell_read_off, out=cell_read_off)
    nrd = np.concatenate(nrd_chunks) if nrd_chunks else np.zeros(0, dtype=np.int64)
    nrd = nrd.astype(np.uint8 if (len(nrd) == 0 or nrd.max() <= 255) else np.uint16)
    pair_snp = np.concatenate(snp_chunks) if snp_chunks else np.zeros(0, dtype=np.int32)
    reads = np.concatenate(rd_chunks) if rd_chunks else np.zeros(0, dtype=np.uint8)
    use_dense = dense_layout and delta >= 1.0
    return SynthPileup(B, S, cell_pair_off, cell_read_off, None if use_dense else pair_snp, nrd, reads,
                       totl, totl.copy(), uniq, truth)


def make_ambient_pileup(rng: np.random.Generator, alleles: np.ndarray, B: int, delta: float, rbar: float, rho,
                        ambient: Optional[np.ndarray] = None, dense_layout: bool = False, chunk_cells: int = 256, quals: Optional[str] = None
                        ) -> Tuple[SynthPileup, np.ndarray, np.ndarray]:
    """Singlet barcodes (cell c is sample c mod V) with ambient contamination: each read comes from the soup with probability rho[c]
    (ALT w.p. a_i) and from the cell otherwise (ALT w.p. its dosage / 2); then sequencing error as in make_pileup.  `rho` is a scalar or
    [B]; `ambient` defaults to the donors' mean dosage / 2; `quals` as in make_pileup.  Returns (pileup, rho[B], a[S])."""
    S, V, _ = alleles.shape
    dosage = np.clip(alleles, 0, 1).sum(axis=2).astype(np.float64)      # [S][V]
    a = dosage.mean(axis=1) / 2.0 if ambient is None else np.asarray(ambient, dtype=np.float64)
    rho = np.broadcast_to(np.asarray(rho, dtype=np.float64), (B,)).copy()
    cell_pair_off = np.zeros(B + 1, dtype=np.int64)
    cell_read_off = np.zeros(B + 1, dtype=np.int64)
    snp_chunks, nrd_chunks, rd_chunks = [], [], []
    totl = np.zeros(B, dtype=np.int32)
    truth = np.full((B, 2), -1, dtype=np.int32)
    for c0 in range(0, B, chunk_cells):
        c1 = min(B, c0 + chunk_cells)
        nc = c1 - c0
        s1 = (np.arange(c0, c1) % V).astype(np.int32)
        truth[c0:c1, 0] = s1
        cov = np.ones((nc, S), dtype=bool) if delta >= 1.0 else rng.random((nc, S)) < delta
        cc, ss = np.nonzero(cov)
        npairs = len(cc)
        nreads = 1 + rng.poisson(max(rbar - 1.0, 0.0), size=npairs)
        pair_of_read = np.repeat(np.arange(npairs), nreads)
        rc, rs = cc[pair_of_read], ss[pair_of_read]
        soup = rng.random(len(rc)) < rho[c0 + rc]
        p_alt = np.where(soup, a[rs], dosage[rs, s1[rc]] / 2.0)
        alt = rng.random(len(rc)) < p_alt
        bq = draw_bq(rng, len(rc), quals)
        e = rng.random(len(rc)) < ERR_OF_BQ[bq]
        u = rng.integers(0, 3, size=len(rc))
        allele = np.where(e, np.where(u == 0, 1 - alt.astype(np.int32), 2), alt.astype(np.int32)).astype(np.uint8)
        keep = allele != 2
        cell_pair_off[c0 + 1:c1 + 1] = np.bincount(cc, minlength=nc)
        cell_read_off[c0 + 1:c1 + 1] = np.bincount(rc[keep], minlength=nc)
        totl[c0:c1] = np.bincount(rc, minlength=nc)
        snp_chunks.append(ss.astype(np.int32))
        nrd_chunks.append(np.bincount(pair_of_read[keep], minlength=npairs))
        rd_chunks.append(((allele[keep] << 7) | bq[keep]).astype(np.uint8))
    np.cumsum(cell_pair_off, out=cell_pair_off)
    np.cumsum(cell_read_off, out=cell_read_off)
    nrd = np.concatenate(nrd_chunks) if nrd_chunks else np.zeros(0, dtype=np.int64)
    nrd = nrd.astype(np.uint8 if (len(nrd) == 0 or nrd.max() <= 255) else np.uint16)
    pair_snp = np.concatenate(snp_chunks) if snp_chunks else np.zeros(0, dtype=np.int32)
    reads = np.concatenate(rd_chunks) if rd_chunks else np.zeros(0, dtype=np.uint8)
    use_dense = dense_layout and delta >= 1.0
    sp = SynthPileup(B, S, cell_pair_off, cell_read_off, None if use_dense else pair_snp, nrd, reads, totl, totl.copy(), totl.copy(), truth)
    return sp, rho, a


def make_ambient_mixed_pileup(rng: np.random.Generator, alleles: np.ndarray, B: int, delta: float, rbar: float, rho, doublet, alpha=0.5,
                              ambient: Optional[np.ndarray] = None, dense_layout: bool = False, chunk_cells: int = 256,
                              quals: Optional[str] = None) -> Tuple[SynthPileup, np.ndarray, np.ndarray, np.ndarray]:
    """Singlets and doublets, each with its own contamination.  Cell c is sample c mod V; where doublet[c] is true a second, different
    sample is drawn and contributes a share alpha[c] of the cell's reads.  Each read comes from the soup with probability rho[c] (ALT
    w.p. a_i), otherwise from the second sample w.p. alpha[c] and from the first elsewise (ALT w.p. the dosage / 2); then sequencing error
    as in make_pileup.  `rho`, `doublet` and `alpha` are scalars or [B]; `ambient` defaults to the donors' mean dosage / 2.  Returns
    (pileup, rho[B], alpha[B], a[S]); pileup.truth[c] = (first, second or -1) and alpha[c] = 0 for singlets."""
    S, V, _ = alleles.shape
    dosage = np.clip(alleles, 0, 1).sum(axis=2).astype(np.float64)      # [S][V]
    a = dosage.mean(axis=1) / 2.0 if ambient is None else np.asarray(ambient, dtype=np.float64)
    rho = np.broadcast_to(np.asarray(rho, dtype=np.float64), (B,)).copy()
    dbl = np.broadcast_to(np.asarray(doublet, dtype=bool), (B,)) & (V > 1)
    alpha = np.where(dbl, np.broadcast_to(np.asarray(alpha, dtype=np.float64), (B,)), 0.0)
    cell_pair_off = np.zeros(B + 1, dtype=np.int64)
    cell_read_off = np.zeros(B + 1, dtype=np.int64)
    snp_chunks, nrd_chunks, rd_chunks = [], [], []
    totl = np.zeros(B, dtype=np.int32)
    truth = np.full((B, 2), -1, dtype=np.int32)
    for c0 in range(0, B, chunk_cells):
        c1 = min(B, c0 + chunk_cells)
        nc = c1 - c0
        s1 = (np.arange(c0, c1) % V).astype(np.int32)
        s2 = ((s1 + 1 + rng.integers(0, max(V - 1, 1), size=nc)) % V).astype(np.int32)
        truth[c0:c1, 0] = s1
        truth[c0:c1, 1] = np.where(dbl[c0:c1], s2, -1)
        cov = np.ones((nc, S), dtype=bool) if delta >= 1.0 else rng.random((nc, S)) < delta
        cc, ss = np.nonzero(cov)
        npairs = len(cc)
        nreads = 1 + rng.poisson(max(rbar - 1.0, 0.0), size=npairs)
        pair_of_read = np.repeat(np.arange(npairs), nreads)
        rc, rs = cc[pair_of_read], ss[pair_of_read]
        soup = rng.random(len(rc)) < rho[c0 + rc]
        src = np.where(rng.random(len(rc)) < alpha[c0 + rc], s2[rc], s1[rc])
        alt = rng.random(len(rc)) < np.where(soup, a[rs], dosage[rs, src] / 2.0)
        bq = draw_bq(rng, len(rc), quals)
        e = rng.random(len(rc)) < ERR_OF_BQ[bq]
        u = rng.integers(0, 3, size=len(rc))
        allele = np.where(e, np.where(u == 0, 1 - alt.astype(np.int32), 2), alt.astype(np.int32)).astype(np.uint8)
        keep = allele != 2
        cell_pair_off[c0 + 1:c1 + 1] = np.bincount(cc, minlength=nc)
        cell_read_off[c0 + 1:c1 + 1] = np.bincount(rc[keep], minlength=nc)
        totl[c0:c1] = np.bincount(rc, minlength=nc)
        snp_chunks.append(ss.astype(np.int32))
        nrd_chunks.append(np.bincount(pair_of_read[keep], minlength=npairs))
        rd_chunks.append(((allele[keep] << 7) | bq[keep]).astype(np.uint8))
    np.cumsum(cell_pair_off, out=cell_pair_off)
    np.cumsum(cell_read_off, out=cell_read_off)
    nrd = np.concatenate(nrd_chunks) if nrd_chunks else np.zeros(0, dtype=np.int64)
    nrd = nrd.astype(np.uint8 if (len(nrd) == 0 or nrd.max() <= 255) else np.uint16)
    pair_snp = np.concatenate(snp_chunks) if snp_chunks else np.zeros(0, dtype=np.int32)
    reads = np.concatenate(rd_chunks) if rd_chunks else np.zeros(0, dtype=np.uint8)
    use_dense = dense_layout and delta >= 1.0
    sp = SynthPileup(B, S, cell_pair_off, cell_read_off, None if use_dense else pair_snp, nrd, reads, totl, totl.copy(), totl.copy(), truth)
    return sp, rho, alpha, a


def make_multiplet_pileup(rng: np.random.Generator, alleles: np.ndarray, B: int, delta: float, rbar: float, kinds, shares,
                          dense_layout: bool = False, quals: Optional[str] = None, chunk_cells: int = 256
                          ) -> Tuple[SynthPileup, np.ndarray, np.ndarray]:
    """Singlets, doublets and triplets.  kinds[c] in {1, 2, 3} is the number of donors of cell c (a scalar or [B]): the first is sample
    c mod V, the others are drawn different from it and from each other.  shares[c] = (w1, w2, w3) (one row or [B][3]) are the donors'
    read shares; the entries of the donors a cell does not have are dropped and the rest scaled to sum 1.  Each read's source is drawn
    by these shares (ALT w.p. its dosage / 2); then sequencing error as in make_pileup.  Returns (pileup, truth3[B][3],
    true_shares[B][3]) with -1 / 0 in the unused donor slots; pileup.truth holds the first two donors."""
    S, V, _ = alleles.shape
    dosage = np.clip(alleles, 0, 1).sum(axis=2).astype(np.float64)      # [S][V]
    kinds = np.broadcast_to(np.asarray(kinds, dtype=np.int64), (B,))
    if B and (kinds.min() < 1 or kinds.max() > 3 or kinds.max() > V):
        raise ValueError(f"kinds: 1, 2 or 3 donors per cell, at most the pool's {V}")
    w = np.broadcast_to(np.asarray(shares, dtype=np.float64), (B, 3)).copy()
    w[np.arange(3)[None, :] >= kinds[:, None]] = 0.0
    if B and (np.any(w < 0.0) or np.any(w.sum(axis=1) <= 0.0)):
        raise ValueError("shares: non-negative, with a positive share among each cell's donors")
    w /= w.sum(axis=1, keepdims=True)
    cum = np.cumsum(w, axis=1)
    cell_pair_off = np.zeros(B + 1, dtype=np.int64)
    cell_read_off = np.zeros(B + 1, dtype=np.int64)
    snp_chunks, nrd_chunks, rd_chunks = [], [], []
    totl = np.zeros(B, dtype=np.int32)
    truth3 = np.full((B, 3), -1, dtype=np.int32)
    for c0 in range(0, B, chunk_cells):
        c1 = min(B, c0 + chunk_cells)
        nc = c1 - c0
        s1 = (np.arange(c0, c1) % V).astype(np.int32)
        s2 = ((s1 + 1 + rng.integers(0, max(V - 1, 1), size=nc)) % V).astype(np.int32)
        k3 = rng.integers(0, max(V - 2, 1), size=nc)                    # the k3-th sample, in cyclic order after s1, that is not s2
        d2 = (s2 - s1) % V
        s3 = ((s1 + 1 + k3 + (1 + k3 >= d2)) % V).astype(np.int32)
        don = np.stack([s1, s2, s3], axis=1)
        truth3[c0:c1] = np.where(np.arange(3)[None, :] < kinds[c0:c1, None], don, -1)
        cov = np.ones((nc, S), dtype=bool) if delta >= 1.0 else rng.random((nc, S)) < delta
        cc, ss = np.nonzero(cov)
        npairs = len(cc)
        nreads = 1 + rng.poisson(max(rbar - 1.0, 0.0), size=npairs)
        pair_of_read = np.repeat(np.arange(npairs), nreads)
        rc, rs = cc[pair_of_read], ss[pair_of_read]
        x = rng.random(len(rc))
        which = np.minimum((x >= cum[c0 + rc, 0]).astype(np.int64) + (x >= cum[c0 + rc, 1]), kinds[c0 + rc] - 1)
        src = don[rc, which]
        alt = rng.random(len(rc)) < dosage[rs, src] / 2.0
        bq = draw_bq(rng, len(rc), quals)
        e = rng.random(len(rc)) < ERR_OF_BQ[bq]
        u = rng.integers(0, 3, size=len(rc))
        allele = np.where(e, np.where(u == 0, 1 - alt.astype(np.int32), 2), alt.astype(np.int32)).astype(np.uint8)
        keep = allele != 2
        cell_pair_off[c0 + 1:c1 + 1] = np.bincount(cc, minlength=nc)
        cell_read_off[c0 + 1:c1 + 1] = np.bincount(rc[keep], minlength=nc)
        totl[c0:c1] = np.bincount(rc, minlength=nc)
        snp_chunks.append(ss.astype(np.int32))
        nrd_chunks.append(np.bincount(pair_of_read[keep], minlength=npairs))
        rd_chunks.append(((allele[keep] << 7) | bq[keep]).astype(np.uint8))
    np.cumsum(cell_pair_off, out=cell_pair_off)
    np.cumsum(cell_read_off, out=cell_read_off)
    nrd = np.concatenate(nrd_chunks) if nrd_chunks else np.zeros(0, dtype=np.int64)
    nrd = nrd.astype(np.uint8 if (len(nrd) == 0 or nrd.max() <= 255) else np.uint16)
    pair_snp = np.concatenate(snp_chunks) if snp_chunks else np.zeros(0, dtype=np.int32)
    reads = np.concatenate(rd_chunks) if rd_chunks else np.zeros(0, dtype=np.uint8)
    use_dense = dense_layout and delta >= 1.0
    sp = SynthPileup(B, S, cell_pair_off, cell_read_off, None if use_dense else pair_snp, nrd, reads, totl, totl.copy(), totl.copy(),
                     truth3[:, :2].copy())
    return sp, truth3, w


def make_pool_pileup(rng: np.random.Generator, alleles: np.ndarray, B: int, delta: float, rbar: float, donor_shares, doublet_rate: float,
                     alpha: float = 0.5, dense_layout: bool = False, quals: Optional[str] = None, chunk_cells: int = 256
                     ) -> Tuple[SynthPileup, dict]:
    """A pool loaded unevenly.  A droplet holds two cells with probability doublet_rate, otherwise one; every cell's donor is an
    independent draw from donor_shares[V] (zeros allowed: a donor of the VCF that is not in the pool), so homotypic doublets occur at
    their natural rate.  In a doublet a read comes from the second cell with probability alpha (ALT w.p. the dosage / 2); then sequencing
    error as in make_pileup.  Returns (pileup, truth): pileup.truth[c] = (first, second or -1), the second equal to the first in a
    homotypic doublet; truth = dict(first[B], second[B] (-1 in singlets), doublet[B] bool, homotypic[B] bool, cell_share[V] = the donors'
    fractions of all drawn cells, doublet_rate = the drawn fraction of droplets with two cells, heterotypic_rate)."""
    S, V, _ = alleles.shape
    dosage = np.clip(alleles, 0, 1).sum(axis=2).astype(np.float64)      # [S][V]
    p = np.asarray(donor_shares, dtype=np.float64)
    if p.shape != (V,) or np.any(p < 0.0) or not p.sum() > 0.0:
        raise ValueError(f"donor_shares: {V} non-negative shares with a positive sum expected")
    p = p / p.sum()
    if not 0.0 <= doublet_rate <= 1.0:
        raise ValueError("doublet_rate must be in [0, 1]")
    first = rng.choice(V, size=B, p=p).astype(np.int32)
    dbl = rng.random(B) < doublet_rate
    second = np.where(dbl, rng.choice(V, size=B, p=p), -1).astype(np.int32)
    cell_pair_off = np.zeros(B + 1, dtype=np.int64)
    cell_read_off = np.zeros(B + 1, dtype=np.int64)
    snp_chunks, nrd_chunks, rd_chunks = [], [], []
    totl = np.zeros(B, dtype=np.int32)
    for c0 in range(0, B, chunk_cells):
        c1 = min(B, c0 + chunk_cells)
        nc = c1 - c0
        s1, s2, isd = first[c0:c1], np.maximum(second[c0:c1], 0), dbl[c0:c1]
        cov = np.ones((nc, S), dtype=bool) if delta >= 1.0 else rng.random((nc, S)) < delta
        cc, ss = np.nonzero(cov)
        npairs = len(cc)
        nreads = 1 + rng.poisson(max(rbar - 1.0, 0.0), size=npairs)
        pair_of_read = np.repeat(np.arange(npairs), nreads)
        rc, rs = cc[pair_of_read], ss[pair_of_read]
        src = np.where(isd[rc] & (rng.random(len(rc)) < alpha), s2[rc], s1[rc])
        alt = rng.random(len(rc)) < dosage[rs, src] / 2.0
        bq = draw_bq(rng, len(rc), quals)
        e = rng.random(len(rc)) < ERR_OF_BQ[bq]
        u = rng.integers(0, 3, size=len(rc))
        allele = np.where(e, np.where(u == 0, 1 - alt.astype(np.int32), 2), alt.astype(np.int32)).astype(np.uint8)
        keep = allele != 2
        cell_pair_off[c0 + 1:c1 + 1] = np.bincount(cc, minlength=nc)
        cell_read_off[c0 + 1:c1 + 1] = np.bincount(rc[keep], minlength=nc)
        totl[c0:c1] = np.bincount(rc, minlength=nc)
        snp_chunks.append(ss.astype(np.int32))
        nrd_chunks.append(np.bincount(pair_of_read[keep], minlength=npairs))
        rd_chunks.append(((allele[keep] << 7) | bq[keep]).astype(np.uint8))
    np.cumsum(cell_pair_off, out=cell_pair_off)
    np.cumsum(cell_read_off, out=cell_read_off)
    nrd = np.concatenate(nrd_chunks) if nrd_chunks else np.zeros(0, dtype=np.int64)
    nrd = nrd.astype(np.uint8 if (len(nrd) == 0 or nrd.max() <= 255) else np.uint16)
    pair_snp = np.concatenate(snp_chunks) if snp_chunks else np.zeros(0, dtype=np.int32)
    reads = np.concatenate(rd_chunks) if rd_chunks else np.zeros(0, dtype=np.uint8)
    use_dense = dense_layout and delta >= 1.0
    sp = SynthPileup(B, S, cell_pair_off, cell_read_off, None if use_dense else pair_snp, nrd, reads, totl, totl.copy(), totl.copy(),
                     np.stack([first, second], axis=1).astype(np.int32))
    cells = np.bincount(first, minlength=V) + np.bincount(second[dbl], minlength=V)
    hom = dbl & (second == first)
    truth = dict(first=first, second=second, doublet=dbl, homotypic=hom, cell_share=cells / max(int(cells.sum()), 1),
                 doublet_rate=float(dbl.mean()) if B else 0.0, heterotypic_rate=float((dbl & ~hom).mean()) if B else 0.0)
    return sp, truth


def barcode_name(i: int) -> str:
    """Deterministic 16-mer barcode whose byte-wise sort order is NOT the id order (exercises the sorted-output rule)."""
    x = (i * 2654435761 + 12345) & 0xFFFFFFFF
    s = []
    for _ in range(16):
        s.append("ACGT"[x & 3])
        x = (x >> 2) | ((x & 3) << 30)
    return "".join(s) + "-1"


def pileup_to_events(rng: np.random.Generator, sp: SynthPileup, shuffle: bool = True, dup_rate: float = 0.1,
                     other_rate: float = 0.03, extra_read_rate: float = 0.2):
    """Turn a CSR pileup into a BAM-ordered event list for the UMI-store path (row a1): UMIs are strings whose sort
    order differs from arrival order, a fraction of reads are PCR duplicates (same UMI, possibly a different base —
    the first one must win), some reads carry allele 2, and some reads overlap no SNP (RD.TOTL only).
    Returns (barcode list, snp, umi list, allele, bq, newread)."""
    B = sp.n_cells
    bcs, snps, umis, als, bqs = [], [], [], [], []
    for c in range(B):
        p0, p1 = int(sp.cell_pair_off[c]), int(sp.cell_pair_off[c + 1])
        r = int(sp.cell_read_off[c])
        for p in range(p0, p1):
            snp = int(sp.pair_snp[p]) if sp.pair_snp is not None else p - p0
            n = int(sp.pair_nrd[p])
            ids = rng.permutation(n + 2)[:n] if n else []
            for t in range(n):
                byte = int(sp.reads[r + t])
                umi = f"U{int(ids[t]) * 7919 % 1000:03d}{'ACGT'[int(ids[t]) % 4]}"
                bcs.append(c); snps.append(snp); umis.append(umi); als.append(byte >> 7); bqs.append(byte & 0x7F)
                if rng.random() < dup_rate:        # PCR duplicate arriving later with a different observation
                    bcs.append(c); snps.append(snp); umis.append(umi); als.append(int(rng.integers(0, 3))); bqs.append(int(rng.integers(13, 41)))
            if n == 0 or rng.random() < other_rate:  # an "other base" read: keeps the pair alive, never enters a likelihood
                bcs.append(c); snps.append(snp); umis.append(f"X{len(umis) % 97:02d}"); als.append(2); bqs.append(int(rng.integers(13, 41)))
            r += n
    n_ev = len(bcs)
    order = rng.permutation(n_ev) if shuffle else np.arange(n_ev)
    # duplicates must stay AFTER their original: keep relative order of equal (cell,snp,umi) keys
    seq = np.empty(n_ev, dtype=np.int64)
    for pos, e in enumerate(order):
        seq[e] = pos
    groups = {}
    for e in range(n_ev):
        groups.setdefault((bcs[e], snps[e], umis[e]), []).append(e)
    for k, es in groups.items():
        if len(es) > 1:
            ps = sorted(seq[e] for e in es)
            for e, p in zip(es, ps):
                seq[e] = p
    order = np.argsort(seq, kind="stable")
    names = [barcode_name(c) for c in range(B)]
    out_bc, out_snp, out_umi, out_al, out_bq, out_new = [], [], [], [], [], []
    for e in order:
        out_bc.append(names[bcs[e]]); out_snp.append(snps[e]); out_umi.append(umis[e]); out_al.append(als[e]); out_bq.append(bqs[e])
        out_new.append(0 if rng.random() < 0.1 else 1)   # 0: same read as the previous event (a read spanning two SNPs)
        if rng.random() < extra_read_rate:   # a read of the same cell that overlaps no SNP
            out_bc.append(names[bcs[e]]); out_snp.append(-1); out_umi.append("."); out_al.append(0); out_bq.append(0); out_new.append(1)
    return (out_bc, np.array(out_snp, dtype=np.int32), out_umi, np.array(out_al, dtype=np.uint8),
            np.array(out_bq, dtype=np.uint8), np.array(out_new, dtype=np.uint8))
