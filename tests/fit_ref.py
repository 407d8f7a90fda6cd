"""float64 numpy restatement of the goodness of fit of a call (dmx_engine_fit), shared by tests/test_fit_cpu.py and
tests/test_gpu_fit.py, and two pool helpers.

Per pair of a used barcode, with its first m = min(n, M) stored reads: every one of the 2^m allele patterns y is enumerated, F_c(y) is
the product of the reads' factors in stored order, L(y) the sum over the components in component order; S0, S1, S2 run over y ascending.
A barcode's pairs are dealt to 64 serial sums (pair k to sum k mod 64) which are then added serially, as include/dmx.h states.  With
longdouble=True every operation (tables, products, sums, logs) is carried out in np.longdouble: the difference to the float64 run is the
restatement's own rounding drift, which sizes the GPU tests' tolerance."""
import numpy as np

import ambient_ref


def host_pairs(cell_pair_off, pair_snp, pair_nrd):
    """(cell, snp, nrd, start, k) per pair: start = the pair's first read byte, k = the pair's index within its barcode."""
    cell, snp, nrd, start = ambient_ref.host_pairs(cell_pair_off, pair_snp, pair_nrd)
    return cell, snp, nrd, start, np.arange(len(cell)) - np.asarray(cell_pair_off, dtype=np.int64)[cell]


def components(g1, g2, alpha, dt):
    """(W[P][NC], cm[P][NC]) of singlets (g2 None: NC = 3) or doublets (NC = 9, l-major, m-minor)."""
    if g2 is None:
        return g1.astype(dt), np.broadcast_to(np.array([0.0, 0.5, 1.0], dtype=dt), g1.shape)
    W = np.stack([g1[:, l].astype(dt) * g2[:, m].astype(dt) for l in range(3) for m in range(3)], axis=1)
    al = alpha.astype(dt)
    cm = np.stack([dt(0.5 * l) + dt((m - l) * 0.5) * al for l in range(3) for m in range(3)], axis=1)
    return W, cm


def pattern_likelihoods(W, p, bq, mat, e3):
    """L[P][2^m]: the likelihood of every allele pattern of m reads (bq[P][m]) under components of weights W[P][NC] and ALT shares p[P][NC]."""
    P, m = bq.shape
    q = 1.0 - p
    mt, et = mat[bq][:, :, None], e3[bq][:, :, None]
    t = np.stack([mt * q[:, None, :] + et * p[:, None, :], et * q[:, None, :] + mt * p[:, None, :]], axis=3)      # [P][m][NC][2]
    L = np.zeros((P, 1 << m), dtype=W.dtype)
    for y in range(1 << m):
        F = t[:, 0, :, y & 1]
        for r in range(1, m):
            F = F * t[:, r, :, (y >> r) & 1]
        s = W[:, 0] * F[:, 0]
        for c in range(1, W.shape[1]):
            s = s + W[:, c] * F[:, c]
        L[:, y] = s
    return L


def pair_moments(L, x):
    """(c0, e1, var, zero, Pr[P][2^m]) per pair from L[P][2^m] and the observed patterns x[P]."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Lx = L[np.arange(len(x)), x]
        c0 = np.log(Lx)
        S0 = np.zeros_like(c0); S1 = np.zeros_like(c0); S2 = np.zeros_like(c0)
        for y in range(L.shape[1]):
            Ly = L[:, y]
            nz = Ly != 0
            u = np.log(Ly) - c0
            S0 = np.where(nz, S0 + Ly, S0)
            S1 = np.where(nz, S1 + Ly * u, S1)
            S2 = np.where(nz, S2 + Ly * (u * u), S2)
        zero = (Lx == 0) | (S0 == 0) | ~np.isfinite(S0)
        e1 = S1 / S0
        d = S2 / S0 - e1 * e1
    return c0, e1, np.where(d > 0, d, 0), zero, L / S0[:, None]


def ref_fit(cell_pair_off, pair_snp, pair_nrd, reads, hyp, alpha, rho, a, g, M, mat, err, longdouble=False, pairs=False):
    """dict of obs / mean / var (dtype float64, or longdouble) and n_snp / n_read / n_trunc / n_zero [B] of the restatement.  pairs=True adds
    "pairs": per counted pair (pair index, c0, e1, var, Pr[2^m]) for the brute-force test."""
    dt = np.longdouble if longdouble else np.float64
    B = len(cell_pair_off) - 1
    cell, snp, nrd, start, k = host_pairs(cell_pair_off, pair_snp, pair_nrd)
    hyp = np.asarray(hyp, dtype=np.int64).reshape(B, 2)
    alpha = np.asarray(alpha, dtype=np.float64)
    rho = np.zeros(B) if rho is None else np.asarray(rho, dtype=np.float64)
    g = np.asarray(g, dtype=np.float32)
    a = np.zeros(g.shape[0]) if a is None else np.asarray(a, dtype=np.float64)
    mat = np.asarray(mat, dtype=np.float64)[:128].astype(dt)
    e3 = np.asarray(err, dtype=np.float64)[:128] / 3.0
    e3 = e3.astype(dt)
    reads = np.asarray(reads)
    v1, v2 = hyp[cell, 0], hyp[cell, 1]
    dbl = v2 >= 0
    keep = (v1 >= 0) & (nrd > 0)
    keep &= (g[snp, np.maximum(v1, 0)] != 0).any(axis=1)
    keep &= ~dbl | (g[snp, np.maximum(v2, 0)] != 0).any(axis=1)
    m = np.minimum(nrd, M)
    P = len(cell)
    c0 = np.zeros(P, dtype=dt); e1 = np.zeros(P, dtype=dt); vr = np.zeros(P, dtype=dt)
    state = np.zeros(P, dtype=np.int8)              # 1 = counted, 2 = zero
    detail = []
    for d_ in (False, True):
        for mm in range(1, M + 1):
            sel = np.flatnonzero(keep & (dbl == d_) & (m == mm))
            if not len(sel):
                continue
            W, cm = components(g[snp[sel], v1[sel]], g[snp[sel], v2[sel]] if d_ else None, alpha[cell[sel]], dt)
            rh = rho[cell[sel]].astype(dt)
            p = (dt(1.0) - rh)[:, None] * cm + (rh * a[snp[sel]].astype(dt))[:, None]
            b = reads[start[sel][:, None] + np.arange(mm)[None, :]].astype(np.int64)
            x = ((b >> 7) << np.arange(mm)[None, :]).sum(axis=1)
            L = pattern_likelihoods(W, p, b & 127, mat, e3)
            c, e, v, zero, pr = pair_moments(L, x)
            c0[sel] = c; e1[sel] = e; vr[sel] = v
            state[sel] = np.where(zero, 2, 1)
            if pairs:
                detail += [(int(sel[i]), c[i], e[i], v[i], pr[i]) for i in range(len(sel)) if not zero[i]]
    cnt = np.flatnonzero(state == 1)
    lanes = np.zeros((3, B, 64), dtype=dt)
    np.add.at(lanes[0], (cell[cnt], k[cnt] % 64), c0[cnt])           # unbuffered, in pair order: each of the 64 sums is serial
    np.add.at(lanes[1], (cell[cnt], k[cnt] % 64), c0[cnt] + e1[cnt])
    np.add.at(lanes[2], (cell[cnt], k[cnt] % 64), vr[cnt])
    tot = np.zeros((3, B), dtype=dt)
    for l in range(64):
        tot = tot + lanes[:, :, l]
    out = dict(obs=tot[0], mean=tot[1], var=tot[2])
    out["n_snp"] = np.bincount(cell[cnt], minlength=B).astype(np.int32)
    out["n_read"] = np.bincount(cell[cnt], weights=m[cnt], minlength=B).astype(np.int32)
    out["n_trunc"] = np.bincount(cell[cnt], weights=(nrd[cnt] > M), minlength=B).astype(np.int32)
    out["n_zero"] = np.bincount(cell[state == 2], minlength=B).astype(np.int32)
    if pairs:
        out["pairs"] = sorted(detail, key=lambda t: t[0])
    return out


def zscore(r):
    """Z = (obs - mean) / sqrt(var) per barcode (nan where var = 0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r["var"] > 0, (r["obs"] - r["mean"]) / np.sqrt(r["var"]), np.nan).astype(np.float64)


def drift(r64, rld):
    """max over obs / mean / var and the barcodes of |float64 - longdouble| / max(1, |longdouble|)."""
    d = 0.0
    for key in ("obs", "mean", "var"):
        x, y = r64[key].astype(np.longdouble), rld[key]
        ok = np.isfinite(y)
        if ok.any():
            d = max(d, float(np.max(np.abs(x[ok] - y[ok]) / np.maximum(1.0, np.abs(y[ok])))))
    return d


def tolerance(r64, rld):
    """The GPU tests' bound on obs / mean / var, relative to max(1, |value|): max(1e-9, 100 x the restatement's own drift)."""
    return max(1e-9, 100.0 * drift(r64, rld))


def scaled_difference(x, y):
    """max |x - y| / max(1, |y|); equal values (and two NaN) count as 0."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    both_nan = np.isnan(x) & np.isnan(y)
    with np.errstate(invalid="ignore"):
        d = np.abs(x - y) / np.maximum(1.0, np.abs(y))
    d = np.where(both_nan | (x == y), 0.0, d)
    return float(np.max(d)) if d.size else 0.0


# ---- pools ------------------------------------------------------------------------------------------------------------------------------

def dropped_donor_pool(rng, synth, geno, S, V, B, delta, rbar, drop=0):
    """A pool of V donors (singlets only) whose donor `drop` is missing from the genotype matrix.  `geno` maps raw alleles [S][2] to a
    float32 [S][3] row (engine.geno_from_gt with its error).  Returns (pileup, g[S][V - 1][3], truth[B]): truth is the barcode's column in
    g, or -1 for the cells of the dropped donor."""
    raw = synth.make_raw_genotypes(rng, S, V)
    sp = synth.make_pileup(rng, raw.alleles, B, delta, rbar, doublet_rate=0.0)
    kept = [v for v in range(V) if v != drop]
    g = np.stack([geno(raw.alleles[:, v]) for v in kept], axis=1).astype(np.float32)
    col = np.full(V, -1, dtype=np.int32)
    col[kept] = np.arange(V - 1)
    return sp, g, col[sp.truth[:, 0]]


def best_other_donor(sp, g, cells, mat, err):
    """For each of `cells`: the column of g with the largest untruncated log-likelihood (obs at M = 8 on every column in turn)."""
    B, Vg = sp.n_cells, g.shape[1]
    ll = np.full((len(cells), Vg), -np.inf)
    for v in range(Vg):
        hyp = np.full((B, 2), -1, dtype=np.int32)
        hyp[cells, 0] = v
        ll[:, v] = ref_fit(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, hyp, np.zeros(B), None, None, g, 8, mat, err)["obs"][cells]
    return ll.argmax(axis=1).astype(np.int32)


def dropped_donor_hypotheses(sp, g, truth, mat, err):
    """hyp[B][2]: the true donor for the barcodes that have one, the best remaining donor for the cells of the dropped one."""
    B = sp.n_cells
    hyp = np.stack([truth, np.full(B, -1)], axis=1).astype(np.int32)
    miss = np.flatnonzero(truth < 0)
    hyp[miss, 0] = best_other_donor(sp, g, miss, mat, err)
    return hyp


def model_drawn_pool(rng, synth, g, B, delta, rbar, hyp, alpha, M=8):
    """B barcodes whose reads are drawn from the model itself: every barcode covers each SNP with probability delta with 1 + Poisson(rbar - 1)
    reads (at most M, so that nothing is truncated) of quality U{13..40}; the pair's component is drawn from the gp rows of the barcode's
    hypothesis (row sums normalised) and every read's allele from the component's law GIVEN that the read is stored.  Returns a SynthPileup."""
    S = g.shape[0]
    err = synth.ERR_OF_BQ
    mat, e3 = 1.0 - err, err / 3.0
    gd = g.astype(np.float64)
    po, ro, snps, nrds, rds = [0], [0], [], [], []
    for b in range(B):
        ss = np.flatnonzero(rng.random(S) < delta)
        n = np.minimum(1 + rng.poisson(max(rbar - 1.0, 0.0), size=len(ss)), M)
        v1, v2 = hyp[b]
        w1 = gd[ss, v1] / gd[ss, v1].sum(axis=1, keepdims=True)
        l = (rng.random(len(ss))[:, None] > np.cumsum(w1, axis=1)).sum(axis=1).clip(0, 2)
        if v2 >= 0:
            w2 = gd[ss, v2] / gd[ss, v2].sum(axis=1, keepdims=True)
            k = (rng.random(len(ss))[:, None] > np.cumsum(w2, axis=1)).sum(axis=1).clip(0, 2)
            p = 0.5 * l + (k - l) * 0.5 * alpha[b]
        else:
            p = 0.5 * l
        pr = np.repeat(p, n)
        bq = rng.integers(13, 41, size=len(pr))
        tA = e3[bq] * (1 - pr) + mat[bq] * pr
        tR = mat[bq] * (1 - pr) + e3[bq] * pr
        alt = (rng.random(len(pr)) < tA / (tA + tR)).astype(np.uint8)
        snps.append(ss.astype(np.int32)); nrds.append(n); rds.append(((alt << 7) | bq).astype(np.uint8))
        po.append(po[-1] + len(ss)); ro.append(ro[-1] + int(n.sum()))
    t = np.ones(B, dtype=np.int32)
    return synth.SynthPileup(B, S, np.array(po, dtype=np.int64), np.array(ro, dtype=np.int64), np.concatenate(snps), np.concatenate(nrds).astype(np.uint8),
                             np.concatenate(rds), t, t.copy(), t.copy(), np.asarray(hyp, dtype=np.int32).copy())
