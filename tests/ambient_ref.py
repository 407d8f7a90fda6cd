"""float64 numpy restatement of the ambient contamination profile (dmx_engine_ambient), shared by
tests/test_ambient_cpu.py and tests/test_gpu_ambient.py.

Per pair of an assigned barcode: S_g[q] = sum over the pair's reads of log(pR (1 - p_g) + pA p_g), p_g = (1 - rho_q) g / 2 + rho_q a_i,
term[q] = logsumexp_g(log gp_g + S_g[q]); LL[b] = the terms of b's pairs added one after another in stored order.  Pairs with no read
or an all-zero gp row are skipped and not counted.  Working in logs, it never underflows."""
import numpy as np


def host_pairs(cell_pair_off, pair_snp, pair_nrd):
    """(cell, snp, nrd, start) per pair: start = the pair's first read byte (reads are stored pair after pair)."""
    po = np.asarray(cell_pair_off, dtype=np.int64)
    cell = np.repeat(np.arange(len(po) - 1), np.diff(po))
    snp = np.asarray(pair_snp, dtype=np.int64) if pair_snp is not None else np.arange(len(cell)) - po[cell]
    nrd = np.asarray(pair_nrd, dtype=np.int64)
    start = np.cumsum(nrd) - nrd
    return cell, snp, nrd, start


def pair_log_factors(nrd, start, reads, a_pair, grid, mat, err):
    """float64 [P][3][Q]: sum over each pair's reads of log(pR (1 - p_g) + pA p_g)."""
    P, Q = len(nrd), len(grid)
    rho = np.asarray(grid, dtype=np.float64)[None, None, :]
    gg = np.arange(3, dtype=np.float64)[None, :, None]
    p = (1.0 - rho) * gg / 2.0 + rho * np.asarray(a_pair, dtype=np.float64)[:, None, None]       # [P][3][Q]
    out = np.zeros((P, 3, Q))
    comp = np.zeros((P, 3, Q))              # Neumaier compensation: a pair of thousands of reads at quality 127 sums to ~-1e5, where a
    e3 = err / 3.0                          # plain running sum would be off by ~1e-9 (one rounding of ulp(1e5) / 2 per read)
    for r in range(int(nrd.max()) if P else 0):
        idx = np.flatnonzero(nrd > r)
        b = reads[start[idx] + r].astype(np.int64)
        bq, alt = b & 127, (b >> 7) != 0
        pR = np.where(alt, e3[bq], mat[bq])[:, None, None]
        pA = np.where(alt, mat[bq], e3[bq])[:, None, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.log(pR * (1.0 - p[idx]) + pA * p[idx])
            s = out[idx]
            t = s + x
            c = np.where(np.abs(s) >= np.abs(x), (s - t) + x, (x - t) + s)
        comp[idx] += np.where(np.isfinite(c), c, 0.0)
        out[idx] = t
    return out + comp


def ref_profile(cell_pair_off, pair_snp, pair_nrd, reads, assign, g, a, grid, mat, err, chunk=4096):
    """(LL[B][Q] f64, n_snp[B], n_read[B]) of the restatement."""
    B = len(cell_pair_off) - 1
    cell, snp, nrd, start = host_pairs(cell_pair_off, pair_snp, pair_nrd)
    assign = np.asarray(assign)
    g = np.asarray(g, dtype=np.float32)
    v = assign[cell] if len(cell) else np.zeros(0, dtype=np.int64)
    keep = (v >= 0) & (nrd > 0)
    rows = g[snp[keep], v[keep]].astype(np.float64) if keep.any() else np.zeros((0, 3))
    sel = np.flatnonzero(keep)[(rows != 0).any(axis=1)]
    Q = len(grid)
    LL = np.zeros((B, Q))
    n_snp = np.zeros(B, dtype=np.int64)
    n_read = np.zeros(B, dtype=np.int64)
    np.add.at(n_snp, cell[sel], 1)
    np.add.at(n_read, cell[sel], nrd[sel])
    reads = np.asarray(reads)
    a = np.asarray(a, dtype=np.float64)
    for k0 in range(0, len(sel), chunk):
        s = sel[k0:k0 + chunk]
        lf = pair_log_factors(nrd[s], start[s], reads, a[snp[s]], grid, mat, err)
        with np.errstate(divide="ignore"):
            x = np.log(g[snp[s], v[s]].astype(np.float64))[:, :, None] + lf                 # [P][3][Q]
        m = x.max(axis=1, keepdims=True)
        mf = np.where(np.isfinite(m), m, 0.0)
        with np.errstate(divide="ignore"):
            term = np.log(np.exp(x - mf).sum(axis=1)) + mf[:, 0, :]
        np.add.at(LL, cell[s], term)            # unbuffered, in index order: each barcode's terms one after another
    return LL, n_snp, n_read
