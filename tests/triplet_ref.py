"""float64 numpy restatement of the triplet profile (dmx_engine_triplet), shared by tests/test_triplet_cpu.py and
tests/test_gpu_triplet.py.

Per pair of a barcode and share triple (w1, w2, w3): S_lmn = sum over the pair's reads of log(pR (1 - p_lmn) + pA p_lmn),
p_lmn = 0.5 (w1 l + w2 m + w3 n); per base pair (v1, v2): log u_n = logsumexp_{l,m}(log gp1_l + log gp2_m + S_lmn), the nine terms added
l-major, m-minor; per third donor c: term = logsumexp_n(log gp_c[n] + log u_n), n ascending; LL[b][s][t][c] = the terms of b's pairs added
one after another in stored order.  Pairs with no read, or where the row of v1 or v2 is all zero, are skipped for the slot; pairs where the
row of c is all zero are skipped for c; neither is counted.  Working in logs, it never underflows."""
import numpy as np

from ambient_ref import host_pairs


def mix_fractions(w):
    """p_lmn = 0.5 (w1 l + w2 m + w3 n), [27] with n fastest."""
    w1, w2, w3 = (float(x) for x in w)
    return np.array([0.5 * (w1 * l + w2 * m + w3 * n) for l in range(3) for m in range(3) for n in range(3)], dtype=np.float64)


def pair_log_factors27(nrd, start, reads, w, mat, err):
    """float64 [P][27]: sum over each pair's reads of log(pR (1 - p_lmn) + pA p_lmn), Neumaier-compensated as ambient_ref.pair_log_factors."""
    P = len(nrd)
    p = mix_fractions(w)[None, :]
    out = np.zeros((P, 27))
    comp = np.zeros((P, 27))
    e3 = err / 3.0
    for r in range(int(nrd.max()) if P else 0):
        idx = np.flatnonzero(nrd > r)
        b = reads[start[idx] + r].astype(np.int64)
        bq, alt = b & 127, (b >> 7) != 0
        pR = np.where(alt, e3[bq], mat[bq])[:, None]
        pA = np.where(alt, mat[bq], e3[bq])[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.log(pR * (1.0 - p) + pA * p)
            s = out[idx]
            t = s + x
            c = np.where(np.abs(s) >= np.abs(x), (s - t) + x, (x - t) + s)
        comp[idx] += np.where(np.isfinite(c), c, 0.0)
        out[idx] = t
    return out + comp


def _lse_ordered(x, axis):
    """log(sum exp(x)) along `axis`, the terms added in index order after the maximum is taken out."""
    x = np.moveaxis(x, axis, 0)
    m = x.max(axis=0)
    mf = np.where(np.isfinite(m), m, 0.0)
    ex = np.exp(x - mf[None])
    tot = ex[0]
    for k in range(1, len(ex)):
        tot = tot + ex[k]
    with np.errstate(divide="ignore"):
        return np.log(tot) + mf


def ref_triplet_profile(cell_pair_off, pair_snp, pair_nrd, reads, base, g, shares, mat, err, chunk=2048):
    """(LL[B][C][T][V] f64, n_snp[B][C][V], n_read[B][C][V]) of the restatement; base[B][C][2], v1 = -1 = slot unused."""
    B = len(cell_pair_off) - 1
    base = np.asarray(base).reshape(B, -1, 2)
    shares = np.asarray(shares, dtype=np.float64).reshape(-1, 3)
    g = np.asarray(g, dtype=np.float32)
    V = g.shape[1]
    Cn, T = base.shape[1], len(shares)
    cell, snp, nrd, start = host_pairs(cell_pair_off, pair_snp, pair_nrd)
    reads = np.asarray(reads)
    LL = np.zeros((B, Cn, T, V))
    n_snp = np.zeros((B, Cn, V), dtype=np.int64)
    n_read = np.zeros((B, Cn, V), dtype=np.int64)
    any_used = (base[:, :, 0] >= 0).any(axis=1)
    sel = np.flatnonzero((nrd > 0) & any_used[cell]) if len(cell) else np.zeros(0, dtype=np.int64)
    for k0 in range(0, len(sel), chunk):
        s = sel[k0:k0 + chunk]
        gs = g[snp[s]].astype(np.float64)                                       # [P][V][3]
        col_ok = (gs != 0).any(axis=2)                                          # [P][V]
        with np.errstate(divide="ignore"):
            lgs = np.log(gs)
        for ti in range(T):
            lf = pair_log_factors27(nrd[s], start[s], reads, shares[ti], mat, err).reshape(-1, 9, 3)      # [P][lm][n]
            for c in range(Cn):
                v1, v2 = base[cell[s], c, 0], base[cell[s], c, 1]
                ok = v1 >= 0
                r = np.arange(len(s))
                g1, g2 = gs[r, np.where(ok, v1, 0)], gs[r, np.where(ok, v2, 0)]
                ok &= (g1 != 0).any(axis=1) & (g2 != 0).any(axis=1)
                if not ok.any():
                    continue
                t = s[ok]
                with np.errstate(divide="ignore"):
                    lw = (np.log(g1[ok])[:, :, None] + np.log(g2[ok])[:, None, :]).reshape(-1, 9)         # l-major, m-minor
                lu = _lse_ordered(lw[:, :, None] + lf[ok], 1)                   # [P'][3]
                term = _lse_ordered(lgs[ok] + lu[:, None, :], 2)                # [P'][V]
                on = col_ok[ok]
                np.add.at(LL[:, c, ti, :], cell[t], np.where(on, term, 0.0))    # unbuffered, in index order: a barcode's terms one after another
                if ti == 0:
                    np.add.at(n_snp[:, c, :], cell[t], on.astype(np.int64))
                    np.add.at(n_read[:, c, :], cell[t], on * nrd[t][:, None])
    return LL, n_snp, n_read
