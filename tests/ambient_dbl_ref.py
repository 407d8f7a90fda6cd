"""float64 numpy restatement of the ambient-aware doublet profile (dmx_engine_ambient_doublet), shared by
tests/test_ambient_dbl_cpu.py and tests/test_gpu_ambient_dbl.py.

Per pair of a barcode, alpha and rho: S_lm = sum over the pair's reads of log(pR (1 - p_lm) + pA p_lm),
p_lm = (1 - rho) (0.5 l + (m - l) 0.5 alpha) + rho a_i; per candidate (v1, v2): term = logsumexp_{l,m}(log gp1_l + log gp2_m + S_lm), the
nine terms added l-major, m-minor; LL[b][c][a][q] = the terms of b's pairs added one after another in stored order.  Pairs with no read,
or where either row is all zero, are skipped for that candidate and not counted.  Working in logs, it never underflows."""
import numpy as np

from ambient_ref import host_pairs


def mix_constants(alpha):
    """c_lm = 0.5 l + (m - l) 0.5 alpha, [9] l-major."""
    return np.array([0.5 * l + (m - l) * 0.5 * alpha for l in range(3) for m in range(3)], dtype=np.float64)


def pair_log_factors9(nrd, start, reads, a_pair, grid, alpha, mat, err):
    """float64 [P][9][Q]: sum over each pair's reads of log(pR (1 - p_lm) + pA p_lm), Neumaier-compensated as ambient_ref.pair_log_factors."""
    P, Q = len(nrd), len(grid)
    rho = np.asarray(grid, dtype=np.float64)[None, None, :]
    p = (1.0 - rho) * mix_constants(alpha)[None, :, None] + rho * np.asarray(a_pair, dtype=np.float64)[:, None, None]      # [P][9][Q]
    out = np.zeros((P, 9, Q))
    comp = np.zeros((P, 9, Q))
    e3 = err / 3.0
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


def ref_dbl_profile(cell_pair_off, pair_snp, pair_nrd, reads, cand, g, a, alphas, grid, mat, err, chunk=2048):
    """(LL[B][C][A][Q] f64, n_snp[B][C], n_read[B][C]) of the restatement; cand[B][C][2], v1 = -1 = slot unused."""
    B = len(cell_pair_off) - 1
    cand = np.asarray(cand).reshape(B, -1, 2)
    Cn, A, Q = cand.shape[1], len(alphas), len(grid)
    cell, snp, nrd, start = host_pairs(cell_pair_off, pair_snp, pair_nrd)
    g = np.asarray(g, dtype=np.float32)
    reads = np.asarray(reads)
    a = np.asarray(a, dtype=np.float64)
    LL = np.zeros((B, Cn, A, Q))
    n_snp = np.zeros((B, Cn), dtype=np.int64)
    n_read = np.zeros((B, Cn), dtype=np.int64)
    any_used = (cand[:, :, 0] >= 0).any(axis=1)
    sel = np.flatnonzero((nrd > 0) & any_used[cell]) if len(cell) else np.zeros(0, dtype=np.int64)
    for k0 in range(0, len(sel), chunk):
        s = sel[k0:k0 + chunk]
        for ai, al in enumerate(alphas):
            lf = pair_log_factors9(nrd[s], start[s], reads, a[snp[s]], grid, float(al), mat, err)          # [P][9][Q]
            for c in range(Cn):
                v1, v2 = cand[cell[s], c, 0], cand[cell[s], c, 1]
                ok = v1 >= 0
                g1 = g[snp[s], np.where(ok, v1, 0)].astype(np.float64)
                g2 = g[snp[s], np.where(ok, v2, 0)].astype(np.float64)
                ok &= (g1 != 0).any(axis=1) & (g2 != 0).any(axis=1)
                if not ok.any():
                    continue
                t = s[ok]
                with np.errstate(divide="ignore"):
                    lw = (np.log(g1[ok])[:, :, None] + np.log(g2[ok])[:, None, :]).reshape(-1, 9)      # l-major, m-minor
                x = lw[:, :, None] + lf[ok]
                m = x.max(axis=1, keepdims=True)
                mf = np.where(np.isfinite(m), m, 0.0)
                ex = np.exp(x - mf)
                tot = ex[:, 0, :]
                for k in range(1, 9):
                    tot = tot + ex[:, k, :]
                with np.errstate(divide="ignore"):
                    term = np.log(tot) + mf[:, 0, :]
                np.add.at(LL[:, c, ai, :], cell[t], term)            # unbuffered, in index order: each barcode's terms one after another
                if ai == 0:
                    np.add.at(n_snp[:, c], cell[t], 1)
                    np.add.at(n_read[:, c], cell[t], nrd[t])
    return LL, n_snp, n_read
