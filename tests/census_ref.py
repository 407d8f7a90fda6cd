"""float64 numpy restatement of the donor-share census (Engine.census_step / Engine.census), for the tests.

Every stored read of a group of barcodes is a draw from a mixture of the V donors with shares w:
  d[i][v] = (gp1 / 2 + gp2) / ((gp0 + gp1) + gp2);  A_i = sum over v, ascending, of w[v] d[i][v] (each product and sum rounded);
  P_r = pR (1 - A_i) + pA A_i;  LL = sum log P_r;  acc[v] = sum over pairs of (1 - d[i][v]) sR + d[i][v] sA, sR = sum pR / P_r, sA = sum pA / P_r.
A_i, P_r and the two quotients are formed with the operations the device uses, in its order, so they carry the same bits; the sums over
pairs and reads are taken in extended precision (the device's order is its own, include/dmx.h).  Also here: the plain and SQUAREM drivers
as include/dmx.h states them, a brute-force step that forms every read's V responsibilities, and a generator of pools with known shares."""
import math
from dataclasses import dataclass

import numpy as np

from demuxlet_amd.engine import HostPileup

U = 2.0 ** -52


@dataclass
class Flat:
    """A pileup by pair and by read."""
    n_cells: int
    cell: np.ndarray         # [P] barcode of each pair
    snp: np.ndarray          # [P]
    nrd: np.ndarray          # [P] stored reads
    read_pair: np.ndarray    # [R] pair of each read
    byte: np.ndarray         # [R] (allele << 7) | bq


def flatten(pl) -> Flat:
    po = np.asarray(pl.cell_pair_off, dtype=np.int64)
    B = len(po) - 1
    cell = np.repeat(np.arange(B), np.diff(po))
    P = len(cell)
    snp = np.asarray(pl.pair_snp, dtype=np.int64) if pl.pair_snp is not None else np.arange(P) - po[cell]
    nrd = np.asarray(pl.pair_nrd).astype(np.int64)
    ro = np.asarray(pl.cell_read_off, dtype=np.int64)
    assert np.array_equal(ro, np.concatenate([[0], np.cumsum(np.bincount(cell, weights=nrd, minlength=B))]).astype(np.int64))
    return Flat(B, cell, snp, nrd, np.repeat(np.arange(P), nrd), np.asarray(pl.reads, dtype=np.uint8))


def dosage(g):
    """(d[S][V] float64, valid[S]): a row that does not sum to a positive finite number gets d = 0 and makes its SNP invalid."""
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    den = (g[:, :, 0] + g[:, :, 1]) + g[:, :, 2]
    ok = (den > 0.0) & np.isfinite(den)
    with np.errstate(all="ignore"):
        d = np.where(ok, (g[:, :, 1] * 0.5 + g[:, :, 2]) / np.where(ok, den, 1.0), 0.0)
    return d, ok.all(axis=1)


def ambient_profile(w, d):
    """A_i = sum over v ascending of w[v] d[i][v], products and sums rounded one by one."""
    A = np.zeros(d.shape[0])
    for v in range(d.shape[1]):
        A = A + w[v] * d[:, v]
    return A


def phred(mat, err):
    """{pR, pA} by read byte."""
    b = np.arange(256)
    m, e3 = np.asarray(mat)[b & 127], np.asarray(err)[b & 127] / 3.0
    return np.where(b >> 7, e3, m), np.where(b >> 7, m, e3)


@dataclass
class Step:
    acc: np.ndarray
    ll: float
    n_read: int
    n_pair: int
    abs_log: float           # sum |log P_r|, for the tolerance
    gap: float


def step(fl: Flat, d, valid, member, w, mat, err) -> Step:
    """One pass for the barcodes member[B] (bool) at shares w[V]."""
    V = d.shape[1]
    w = np.asarray(w, dtype=np.float64)
    use = np.asarray(member, dtype=bool)[fl.cell] & (fl.nrd > 0) & valid[fl.snp]
    ru = use[fl.read_pair]
    rp = fl.read_pair[ru]
    if len(rp) == 0:
        return Step(np.zeros(V), 0.0, 0, 0, 0.0, 0.0)
    tR, tA = phred(mat, err)
    pR, pA = tR[fl.byte[ru]], tA[fl.byte[ru]]
    A = ambient_profile(w, d)[fl.snp[rp]]
    with np.errstate(all="ignore"):
        P = pR * (1.0 - A) + pA * A
        P_ = len(fl.cell)
        sR = np.bincount(rp, weights=pR / P, minlength=P_)[use]        # (bincount adds in the order given: the pair's stored order)
        sA = np.bincount(rp, weights=pA / P, minlength=P_)[use]
        lg = np.log(P)
    dd = d[fl.snp[use]]
    terms = (1.0 - dd) * sR[:, None] + dd * sA[:, None]
    acc = terms.sum(axis=0, dtype=np.longdouble).astype(np.float64)
    N = int(len(rp))
    return Step(acc, math.fsum(lg), N, int(use.sum()), math.fsum(np.abs(lg)), N * (acc.max() / N - 1.0))


def step_brute(fl: Flat, d, valid, member, w, mat, err, dtype=np.float64):
    """The same from every read's V responsibilities: f_rv = pR (1 - d_v) + pA d_v, P_r = sum_v w_v f_rv, acc_v = sum_r f_rv / P_r
    (so that w_v acc_v is donor v's expected read count).  Returns (acc, ll) in `dtype`."""
    use = np.asarray(member, dtype=bool)[fl.cell] & (fl.nrd > 0) & valid[fl.snp]
    ru = use[fl.read_pair]
    rp = fl.read_pair[ru]
    tR, tA = phred(mat, err)
    pR, pA = tR[fl.byte[ru]].astype(dtype)[:, None], tA[fl.byte[ru]].astype(dtype)[:, None]
    dr = d[fl.snp[rp]].astype(dtype)
    f = pR * (1 - dr) + pA * dr
    P = f @ np.asarray(w).astype(dtype)
    return (f / P[:, None]).sum(axis=0), np.log(P).sum()


def em_image(w, s: Step):
    return w * s.acc / s.n_read


def extrapolate(w0, w1, w2):
    """SQUAREM's point from three EM iterates, as include/dmx.h states it."""
    r = w1 - w0
    u = (w2 - w1) - r
    rr, uu = float((r * r).sum()), float((u * u).sum())
    a = -math.sqrt(rr) / math.sqrt(uu) if uu > 0.0 else -1.0
    if not (a <= -1.0) or not math.isfinite(a):
        a = -1.0
    while True:
        x = (w0 - 2.0 * a * r) + a * a * u
        if not (x < 0.0).any() or a == -1.0:
            break
        a = 0.5 * (a - 1.0)
        if a > -1.0 - 1e-9:
            a = -1.0
    if a == -1.0:
        x = w2.copy()
    x = np.where(x > 0.0, x, 0.0)
    return x / x.sum()


def run(fl: Flat, d, valid, member, mat, err, w0=None, tol=1e-4, max_steps=2000, accelerate=True, path=None):
    """The driver for one group.  Returns dict(w, ll, gap, n_steps, converged, n_read, n_pair); `path` collects (w, Step) per pass."""
    V = d.shape[1]
    x = np.full(V, 1.0 / V) if w0 is None else np.asarray(w0, dtype=np.float64).copy()
    phase, steps = 0, 0
    a0 = a1 = a2 = None
    ll1 = 0.0
    while True:
        s = step(fl, d, valid, member, x, mat, err)
        steps += 1
        if path is not None:
            path.append((x.copy(), s))
        empty = s.n_read == 0
        conv = empty or (math.isfinite(s.ll) and s.gap <= tol)
        if conv or steps >= max_steps:
            return dict(w=x, ll=0.0 if empty else s.ll, gap=0.0 if empty else s.gap, n_steps=steps, converged=int(conv), n_read=s.n_read,
                        n_pair=s.n_pair)
        if not accelerate:
            x = em_image(x, s)
        elif phase == 0:
            a0, a1 = x, em_image(x, s)
            x, phase = a1, 1
        elif phase == 1:
            ll1, a2 = s.ll, em_image(x, s)
            x, phase = extrapolate(a0, a1, a2), 2
        else:
            x = a2 if (not math.isfinite(s.ll) or s.ll < ll1) else em_image(x, s)
            phase = 0


def gt_rows(alleles, gt_error):
    """gp[S][V][3] float32 of called genotypes: 1 - gt_error on the genotype, gt_error / 2 on the two others."""
    k = np.clip(np.asarray(alleles), 0, 1).sum(axis=2)
    g = np.full(k.shape + (3,), gt_error / 2.0, dtype=np.float32)
    np.put_along_axis(g, k[:, :, None], np.float32(1.0 - gt_error), axis=2)
    return g


def make_pool(rng, alleles, shares, B, n_reads, bq_lo=10, bq_hi=40, cell_shares=None, dense=False, nrd_dtype=np.uint8):
    """Draw n_reads reads: a barcode (uniform, or cell_shares[B]), a SNP (uniform), a donor (shares), one of the donor's two alleles,
    a base quality in [bq_lo, bq_hi]; with probability err(bq) the base is wrong — one time in three it is the other allele, otherwise
    neither (allele 2: not stored).  Returns a sparse (or dense) HostPileup."""
    S, V = alleles.shape[:2]
    cell = rng.choice(B, n_reads, p=cell_shares)
    snp = rng.integers(0, S, n_reads)
    donor = rng.choice(V, n_reads, p=np.asarray(shares) / np.sum(shares))
    al = np.clip(alleles[snp, donor, rng.integers(0, 2, n_reads)], 0, 1)
    bq = rng.integers(bq_lo, bq_hi + 1, n_reads)
    wrong = rng.random(n_reads) < 10.0 ** (-bq / 10.0)
    other = rng.random(n_reads) < 1.0 / 3.0
    keep = ~wrong | other
    al = np.where(wrong, 1 - al, al)
    return build_pileup(B, S, cell[keep], snp[keep], ((al[keep] << 7) | bq[keep]).astype(np.uint8), dense=dense, nrd_dtype=nrd_dtype)


def build_pileup(B, S, cell, snp, byte, dense=False, nrd_dtype=np.uint8, extra_pairs=()):
    """A HostPileup from reads (cell, snp, byte) in any order; reads of one pair keep their order.  extra_pairs: (cell, snp) pairs
    without a stored read (allele 2 only)."""
    cell, snp = np.asarray(cell, dtype=np.int64), np.asarray(snp, dtype=np.int64)
    key = cell * S + snp
    o = np.argsort(key, kind="stable")
    key, byte = key[o], np.asarray(byte, dtype=np.uint8)[o]
    if dense:
        pk = np.arange(B * S, dtype=np.int64)
    else:
        pk = np.unique(np.concatenate([key, np.array([c * S + s for c, s in extra_pairs], dtype=np.int64)]))
    nrd = np.bincount(np.searchsorted(pk, key), minlength=len(pk))
    pc = pk // S
    po = np.concatenate([[0], np.cumsum(np.bincount(pc, minlength=B))]).astype(np.int64)
    ro = np.concatenate([[0], np.cumsum(np.bincount(pc, weights=nrd, minlength=B))]).astype(np.int64)
    tot = np.diff(ro).astype(np.int32)
    assert nrd.max(initial=0) <= np.iinfo(nrd_dtype).max
    return HostPileup(B, S, po, ro, None if dense else (pk % S).astype(np.int32), nrd.astype(nrd_dtype), byte, tot, tot.copy(), tot.copy())


def to_dense(pl):
    fl = flatten(pl)
    return build_pileup(pl.n_cells, pl.n_snps, fl.cell[fl.read_pair], fl.snp[fl.read_pair], fl.byte, dense=True, nrd_dtype=np.uint16)
