"""A serial restatement of the model-drawn null pool (include/dmx.h, dmx_engine_redraw).  Readable, not fast.

Python floats are binary64 and every operation below is rounded on its own, as the contract asks; integers are Python's, reduced mod
2^64.  The source is anything with the attributes of demuxlet_amd.engine.HostPileup."""
import math

import numpy as np

from compose_ref import GOLD, mix64

PAIR, DONOR = 0, 1
TWO32 = 4294967296.0


def read_key(seed: int, cell_id: int) -> int:
    """First-level key of a barcode's read stream."""
    return mix64(seed + GOLD * (4 * cell_id + 1))


def geno_key(mode: int, seed: int, geno_seed: int, cell_id: int, slot: int, sample: int) -> int:
    """First-level key of a genotype stream: PAIR by (seed, barcode id, slot), DONOR by (geno_seed, sample) alone."""
    if mode == DONOR:
        return mix64(geno_seed + GOLD * (4 * sample + 2))
    return mix64(seed + GOLD * (4 * cell_id + 2 + slot))


def uniform32(key: int, snp: int, r: int = 0) -> int:
    return mix64(key + ((snp << 32) | r)) >> 32


def row_ok(row) -> bool:
    w = [float(x) for x in row]
    return all(math.isfinite(x) and x >= 0.0 for x in w) and any(x != 0.0 for x in w)


def genotype_of(row, ug: int) -> int:
    """The genotype of a float32 row (w0, w1, w2) at the 32-bit uniform ug."""
    w0, w1, w2 = (float(np.float32(x)) for x in row)
    c01 = w0 + w1
    s = c01 + w2
    x = (float(ug) * 2.0 ** -32) * s
    return 0 if x < w0 else 1 if x < c01 else 2


def component_share(l: int, m: int, alpha: float) -> float:
    """c_c of dmx_engine_fit: 0.5 g for a singlet (m < 0), 0.5 l + ((m - l) 0.5) alpha for a doublet."""
    if m < 0:
        return 0.5 * l
    return 0.5 * l + (float(m - l) * 0.5) * alpha


def alt_probability(pc: float, mat: float, e3: float, swap: bool = False) -> float:
    """q = (e3 (1 - p_c) + mat p_c) / (mat + e3).  swap=True is the deliberately wrong variant with p_c and 1 - p_c exchanged."""
    q1 = 1.0 - pc
    if swap:
        pc, q1 = q1, pc
    num = e3 * q1 + mat * pc
    den = mat + e3
    return num / den


def threshold(q: float):
    """thr of a probability, or None when the read keeps its allele."""
    if not (q >= 0.0 and q <= 1.0):
        return None
    return int(q * TWO32)


def redraw(src, hyp, alpha, rho, a, g, mat, err, seed: int, geno_seed: int, mode: int, index_base: int = 0, swap: bool = False) -> dict:
    """reads (uint8), geno (int8 [P][2]), the info counts, and q1 [P] (the ALT probability of each drawn pair's first read, nan elsewhere)."""
    B = len(src.cell_pair_off) - 1
    hyp = np.asarray(hyp, dtype=np.int64).reshape(B, 2)
    g = np.asarray(g, dtype=np.float32)
    mat = [float(x) for x in np.asarray(mat, dtype=np.float64)[:128]]
    e3t = [float(x) / 3.0 for x in np.asarray(err, dtype=np.float64)[:128]]
    reads = np.array(src.reads, dtype=np.uint8, copy=True)
    P = len(src.pair_nrd)
    geno = np.full((P, 2), -1, dtype=np.int8)
    qfirst = np.full(P, np.nan)
    info = dict(n_cells=B, n_used=0, n_singlet=0, n_doublet=0, n_pairs_drawn=0, n_pairs_skipped=0, n_reads_drawn=0, n_reads_kept=0)
    for b in range(B):
        v1, v2 = int(hyp[b, 0]), int(hyp[b, 1])
        if v1 < 0:
            continue
        info["n_used"] += 1
        info["n_doublet" if v2 >= 0 else "n_singlet"] += 1
        cid = index_base + b
        rh = float(rho[b]) if rho is not None else 0.0
        om = 1.0 - rh
        al = float(alpha[b])
        kr = read_key(seed, cid)
        k1 = geno_key(mode, seed, geno_seed, cid, 0, v1)
        k2 = geno_key(mode, seed, geno_seed, cid, 1, v2) if v2 >= 0 else 0
        p0, p1 = int(src.cell_pair_off[b]), int(src.cell_pair_off[b + 1])
        off = int(src.cell_read_off[b])
        for p in range(p0, p1):
            n = int(src.pair_nrd[p])
            start, off = off, off + n
            if n == 0:
                continue
            snp = int(src.pair_snp[p]) if src.pair_snp is not None else p - p0
            if not row_ok(g[snp, v1]) or (v2 >= 0 and not row_ok(g[snp, v2])):
                info["n_pairs_skipped"] += 1
                continue
            l = genotype_of(g[snp, v1], uniform32(k1, snp))
            m = genotype_of(g[snp, v2], uniform32(k2, snp)) if v2 >= 0 else -1
            geno[p] = (l, m)
            ra = rh * (float(a[snp]) if a is not None else 0.0)
            pc = om * component_share(l, m, al) + ra
            info["n_pairs_drawn"] += 1
            for r in range(n):
                bq = int(reads[start + r]) & 127
                q = alt_probability(pc, mat[bq], e3t[bq], swap)
                if r == 0:
                    qfirst[p] = q
                thr = threshold(q)
                if thr is None:
                    info["n_reads_kept"] += 1
                    continue
                reads[start + r] = bq | (128 if uniform32(kr, snp, r) < thr else 0)
                info["n_reads_drawn"] += 1
    return dict(reads=reads, geno=geno, q1=qfirst, **info)


def marginal_first_read(src, hyp, alpha, rho, a, g, mat, err, swap: bool = False):
    """Per pair with a stored read and usable rows: (pair index, sum_c W_c q_c / sum_c W_c of its FIRST read) — the law of that read's allele
    in PAIR mode, the genotype integrated out."""
    B = len(src.cell_pair_off) - 1
    hyp = np.asarray(hyp, dtype=np.int64).reshape(B, 2)
    g = np.asarray(g, dtype=np.float32)
    mat = np.asarray(mat, dtype=np.float64)[:128]
    e3t = np.asarray(err, dtype=np.float64)[:128] / 3.0
    idx, prob = [], []
    for b in range(B):
        v1, v2 = int(hyp[b, 0]), int(hyp[b, 1])
        if v1 < 0:
            continue
        rh = float(rho[b]) if rho is not None else 0.0
        p0, p1 = int(src.cell_pair_off[b]), int(src.cell_pair_off[b + 1])
        off = int(src.cell_read_off[b])
        for p in range(p0, p1):
            n = int(src.pair_nrd[p])
            start, off = off, off + n
            if n == 0:
                continue
            snp = int(src.pair_snp[p]) if src.pair_snp is not None else p - p0
            if not row_ok(g[snp, v1]) or (v2 >= 0 and not row_ok(g[snp, v2])):
                continue
            bq = int(src.reads[start]) & 127
            ra = rh * (float(a[snp]) if a is not None else 0.0)
            num = den = 0.0
            for l in range(3):
                for m in (range(3) if v2 >= 0 else (-1,)):
                    W = float(g[snp, v1, l]) * (float(g[snp, v2, m]) if v2 >= 0 else 1.0)
                    pc = (1.0 - rh) * component_share(l, m, float(alpha[b])) + ra
                    num += W * alt_probability(pc, float(mat[bq]), float(e3t[bq]), swap)
                    den += W
            idx.append(p); prob.append(num / den)
    return np.array(idx, dtype=np.int64), np.array(prob)


def first_read_T(src, reads, idx, prob, directed: bool = True) -> float:
    """T = sum s (y - p) / sqrt(sum p (1 - p)) over the first reads of the pairs idx, y the redrawn allele and p its marginal ALT
    probability.  directed: s = +1 where p >= 0.5 and -1 elsewhere — fixed by p alone, so T is standard normal under the law either way,
    but a draw that leans away from its own probability adds up instead of cancelling between REF-leaning and ALT-leaning pairs (the
    plain sum, s = 1, cannot see p_c exchanged with 1 - p_c in a pool with as many of the one as of the other)."""
    starts = np.concatenate([[0], np.cumsum(np.asarray(src.pair_nrd, dtype=np.int64))])[:-1]
    first = np.asarray(src.cell_read_off, dtype=np.int64)[0] + starts
    y = (np.asarray(reads)[first[idx]] >> 7).astype(np.float64)
    s = np.where(prob >= 0.5, 1.0, -1.0) if directed else 1.0
    return float(np.sum(s * (y - prob)) / math.sqrt(np.sum(prob * (1.0 - prob))))


def fit_T(r: dict, used) -> float:
    """T = sum_b (obs_b - mean_b) / sqrt(sum_b var_b) over the used barcodes of a fit result (tests/fit_ref.py or Engine.fit_profile)."""
    u = np.asarray(used, dtype=bool)
    return float(np.sum(np.asarray(r["obs"])[u] - np.asarray(r["mean"])[u]) / math.sqrt(np.sum(np.asarray(r["var"])[u])))


# ---- the pool of the exact-law tests (tests/test_redraw_cpu.py on the restatement, tests/test_gpu_redraw.py on the device) -----------------

LAW_POOL_SEED, LAW_SEED, LAW_GENO_SEED = 20, 1234, 99


def law_pool(synth, geno_from_gt, B=320, S=1500, V=6, delta=0.1, rbar=1.6):
    """B barcodes of ~S delta pairs, 40 % doublets, under their true hypotheses: doublets at alpha 0.5 or 0.3, rho 0 or 0.2 over a soup of
    random ALT frequencies, gp rows softened (0.7 g + 0.1) so that every component has weight.  Returns (pileup, g, hyp, alpha, rho, a)."""
    rng = np.random.default_rng(LAW_POOL_SEED)
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([geno_from_gt(raw.alleles[s], 0.01) for s in range(S)]).astype(np.float32)
    g = (np.float32(0.7) * g + np.float32(0.1)).astype(np.float32)
    sp = synth.make_pileup(rng, raw.alleles, B, delta, rbar, doublet_rate=0.4)
    hyp = sp.truth.astype(np.int32).copy()
    alpha = np.where(hyp[:, 1] >= 0, rng.choice([0.5, 0.3], size=B), 0.0)
    rho = rng.choice([0.0, 0.2], size=B)
    a = rng.uniform(0.0, 1.0, size=S)
    return sp, g, hyp, alpha, rho, a
