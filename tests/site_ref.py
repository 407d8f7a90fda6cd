"""float64 numpy restatement of the site audit (dmx_engine_site_fit), shared by tests/test_site_cpu.py and
tests/test_gpu_site.py, and the swapped-rows pool.

The per-pair terms are tests/fit_ref.py's (pattern_likelihoods, pair_moments), extended by the two ALT-count sums A1 and A2 over y
ascending.  The summation plan is include/dmx.h's: the used barcodes are listed singlet hypotheses first, then doublet hypotheses, each
in ascending cell id; each list is cut into chunks of 64; for a SNP the terms of a chunk's barcodes are added onto +0 in list order, then
the chunk partials onto +0 in ascending chunk order.  With longdouble=True every operation is carried out in np.longdouble: the
difference to the float64 run is the restatement's own rounding drift, which sizes the GPU tests' tolerance (fit_ref.tolerance's rule)."""
import numpy as np

import fit_ref

FLOATS = ("obs", "mean", "var", "exc", "vexc")
COUNTS = ("n_cell", "n_read", "n_alt", "n_trunc", "n_zero")
KEYS = FLOATS + COUNTS
CHUNK = 64


def alt_moments(L):
    """(S0, A1, A2) per pair from L[P][2^m]: over y ascending from +0, a pattern with L(y) = 0 adding nothing."""
    S0 = np.zeros(L.shape[0], dtype=L.dtype); A1 = np.zeros_like(S0); A2 = np.zeros_like(S0)
    for y in range(L.shape[1]):
        Ly = L[:, y]
        nz = Ly != 0
        k = L.dtype.type(bin(y).count("1"))
        S0 = np.where(nz, S0 + Ly, S0)
        A1 = np.where(nz, A1 + Ly * k, A1)
        A2 = np.where(nz, A2 + Ly * (k * k), A2)
    return S0, A1, A2


def listing(hyp):
    """(singlet cell ids, doublet cell ids), each ascending: the order in which dmx_engine_fit lists the used barcodes."""
    hyp = np.asarray(hyp, dtype=np.int64).reshape(-1, 2)
    return np.flatnonzero((hyp[:, 0] >= 0) & (hyp[:, 1] < 0)), np.flatnonzero((hyp[:, 0] >= 0) & (hyp[:, 1] >= 0))


def pair_terms(cell_pair_off, pair_snp, pair_nrd, reads, hyp, alpha, rho, a, g, M, mat, err, longdouble=False):
    """Per pair: dict of cell, snp, nrd, m, state (0 = not counted, 1 = counted, 2 = zero), kx (ALT among the m reads) and the five terms
    c0, c0 + e1, var, exc, vexc (dtype float64 or longdouble)."""
    dt = np.longdouble if longdouble else np.float64
    B = len(cell_pair_off) - 1
    cell, snp, nrd, start, _ = fit_ref.host_pairs(cell_pair_off, pair_snp, pair_nrd)
    hyp = np.asarray(hyp, dtype=np.int64).reshape(B, 2)
    alpha = np.asarray(alpha, dtype=np.float64)
    rho = np.zeros(B) if rho is None else np.asarray(rho, dtype=np.float64)
    g = np.asarray(g, dtype=np.float32)
    a = np.zeros(g.shape[0]) if a is None else np.asarray(a, dtype=np.float64)
    mat = np.asarray(mat, dtype=np.float64)[:128].astype(dt)
    e3 = (np.asarray(err, dtype=np.float64)[:128] / 3.0).astype(dt)
    reads = np.asarray(reads)
    v1, v2 = hyp[cell, 0], hyp[cell, 1]
    dbl = v2 >= 0
    keep = (v1 >= 0) & (nrd > 0)
    keep &= (g[snp, np.maximum(v1, 0)] != 0).any(axis=1)
    keep &= ~dbl | (g[snp, np.maximum(v2, 0)] != 0).any(axis=1)
    m = np.minimum(nrd, M)
    P = len(cell)
    terms = np.zeros((5, P), dtype=dt)
    state = np.zeros(P, dtype=np.int8)
    kx = np.zeros(P, dtype=np.int64)
    for d_ in (False, True):
        for mm in range(1, M + 1):
            sel = np.flatnonzero(keep & (dbl == d_) & (m == mm))
            if not len(sel):
                continue
            W, cm = fit_ref.components(g[snp[sel], v1[sel]], g[snp[sel], v2[sel]] if d_ else None, alpha[cell[sel]], dt)
            rh = rho[cell[sel]].astype(dt)
            p = (dt(1.0) - rh)[:, None] * cm + (rh * a[snp[sel]].astype(dt))[:, None]
            b = reads[start[sel][:, None] + np.arange(mm)[None, :]].astype(np.int64)
            x = ((b >> 7) << np.arange(mm)[None, :]).sum(axis=1)
            L = fit_ref.pattern_likelihoods(W, p, b & 127, mat, e3)
            c0, e1, vr, zero, _ = fit_ref.pair_moments(L, x)
            S0, A1, A2 = alt_moments(L)
            k = (b >> 7).sum(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                a1 = A1 / S0
                da = A2 / S0 - a1 * a1
                da = np.where(da > 0, da, 0)
                terms[0, sel] = c0; terms[1, sel] = c0 + e1; terms[2, sel] = vr         # (pairs counted in n_zero hold non-numbers: never used)
                terms[3, sel] = k.astype(dt) - a1; terms[4, sel] = da
            state[sel] = np.where(zero, 2, 1)
            kx[sel] = k
    return dict(cell=cell, snp=snp, nrd=nrd, m=m, state=state, kx=kx, terms=terms)


def ref_site(cell_pair_off, pair_snp, pair_nrd, reads, hyp, alpha, rho, a, g, M, mat, err, longdouble=False, chunk=CHUNK, lists=None, terms=None):
    """dict of obs / mean / var / exc / vexc [S] (float64, or longdouble) and n_cell / n_read / n_alt / n_trunc / n_zero [S] of the
    restatement.  `chunk` and `lists` (singlet ids, doublet ids in list order) replace the plan's chunk size and list order for the tests
    of the summation plan; `terms` reuses pair_terms' result."""
    dt = np.longdouble if longdouble else np.float64
    S = np.asarray(g).shape[0]
    B = len(cell_pair_off) - 1
    t = terms if terms is not None else pair_terms(cell_pair_off, pair_snp, pair_nrd, reads, hyp, alpha, rho, a, g, M, mat, err, longdouble)
    sng, dbl = listing(hyp) if lists is None else lists
    ncs = -(-len(sng) // chunk)
    nch = ncs + -(-len(dbl) // chunk)
    pos = np.full(B, -1, dtype=np.int64)                      # list position; chunk of a barcode
    pos[sng] = np.arange(len(sng)); pos[dbl] = len(sng) + np.arange(len(dbl))
    chk = np.full(B, -1, dtype=np.int64)
    chk[sng] = np.arange(len(sng)) // chunk; chk[dbl] = ncs + np.arange(len(dbl)) // chunk
    cnt = np.flatnonzero(t["state"] == 1)
    cnt = cnt[np.argsort(pos[t["cell"][cnt]], kind="stable")]   # in list order: np.add.at adds unbuffered, in this order
    partial = np.zeros((5, max(nch, 1), S), dtype=dt)
    for j in range(5):
        np.add.at(partial[j], (chk[t["cell"][cnt]], t["snp"][cnt]), t["terms"][j, cnt])
    tot = np.zeros((5, S), dtype=dt)
    for c in range(nch):
        tot = tot + partial[:, c, :]
    out = {k: tot[j] for j, k in enumerate(FLOATS)}
    sc = t["snp"][cnt]
    out["n_cell"] = np.bincount(sc, minlength=S).astype(np.int32)
    out["n_read"] = np.bincount(sc, weights=t["m"][cnt], minlength=S).astype(np.int32)
    out["n_alt"] = np.bincount(sc, weights=t["kx"][cnt], minlength=S).astype(np.int32)
    out["n_trunc"] = np.bincount(sc, weights=(t["nrd"][cnt] > M), minlength=S).astype(np.int32)
    out["n_zero"] = np.bincount(t["snp"][t["state"] == 2], minlength=S).astype(np.int32)
    return out


def zscore(r, num="obs", den="var", sub="mean"):
    """Z = (obs - mean) / sqrt(var) per SNP (nan where var = 0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r[den] > 0, (r[num] - r[sub]) / np.sqrt(r[den]), np.nan).astype(np.float64)


def zalt(r):
    """Z.ALT = exc / sqrt(vexc) per SNP (nan where vexc = 0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r["vexc"] > 0, r["exc"] / np.sqrt(r["vexc"]), np.nan).astype(np.float64)


def drift(r64, rld):
    """max over the five float outputs and the SNPs of |float64 - longdouble| / max(1, |longdouble|)."""
    d = 0.0
    for key in FLOATS:
        x, y = r64[key].astype(np.longdouble), rld[key]
        ok = np.isfinite(y)
        if ok.any():
            d = max(d, float(np.max(np.abs(x[ok] - y[ok]) / np.maximum(1.0, np.abs(y[ok])))))
    return d


def tolerance(r64, rld):
    """fit_ref's rule: max(1e-9, 100 x the restatement's own drift), relative to max(1, |value|)."""
    return max(1e-9, 100.0 * drift(r64, rld))


scaled_difference = fit_ref.scaled_difference


# ---- the swapped-rows pool --------------------------------------------------------------------------------------------------------------

def swapped_rows_pool(rng, synth, geno, S, V, B, delta, rbar, n_swap):
    """A pool of V donors (singlets only) over S SNPs; the genotype matrix has REF and ALT exchanged in n_swap rows (every donor's row at the
    SNP reversed).  `geno` maps raw alleles [S][2] to float32 [S][3] rows.  Returns (pileup, g[S][V][3], swapped[S] bool, truth[B])."""
    raw = synth.make_raw_genotypes(rng, S, V)
    sp = synth.make_pileup(rng, raw.alleles, B, delta, rbar, doublet_rate=0.0)
    g = np.stack([geno(raw.alleles[:, v]) for v in range(V)], axis=1).astype(np.float32)
    swapped = np.zeros(S, dtype=bool)
    swapped[rng.choice(S, n_swap, replace=False)] = True
    g[swapped] = g[swapped][:, :, ::-1]
    return sp, np.ascontiguousarray(g), swapped, sp.truth[:, 0].copy()


SWAP_M, SWAP_Z_MIN, SWAP_MIN_CELLS = 4, -6.0, 10    # sites.py's defaults


def swap_pool(engine, synth):
    """The swapped-rows pool of both test files: 8 donors, 1 500 SNPs of which 380 have REF and ALT exchanged, 250 singlet barcodes at
    delta = 0.1 (25 cells per SNP, 150 SNPs per barcode), 1.25 reads per pair, near-hard GT rows."""
    return swapped_rows_pool(np.random.default_rng(41), synth, lambda al: engine.geno_from_gt(al, 0.01), 1500, 8, 250, 0.1, 1.25, 380)


def drop_pairs(sp_arrays, mask):
    """(cell_pair_off, pair_snp, pair_nrd, reads) without the pairs at the SNPs of mask[S]."""
    cell_pair_off, pair_snp, pair_nrd, reads = sp_arrays
    cell, snp, nrd, start, _ = fit_ref.host_pairs(cell_pair_off, pair_snp, pair_nrd)
    keep = ~np.asarray(mask, dtype=bool)[snp]
    B = len(cell_pair_off) - 1
    po = np.concatenate([[0], np.cumsum(np.bincount(cell[keep], minlength=B))]).astype(np.int64)
    rkeep = np.repeat(keep, nrd)
    return po, snp[keep].astype(np.int32), np.asarray(pair_nrd)[keep], np.asarray(reads)[rkeep]


def argmax_singlets(sp_arrays, g, M, mat, err, V):
    """The singlet call of every barcode: the donor with the largest obs (fit_ref.ref_fit on every column in turn)."""
    po, ps, pn, rd = sp_arrays
    B = len(po) - 1
    ll = np.full((B, V), -np.inf)
    for v in range(V):
        hyp = np.stack([np.full(B, v), np.full(B, -1)], axis=1)
        r = fit_ref.ref_fit(po, ps, pn, rd, hyp, np.zeros(B), None, None, g, M, mat, err)
        ll[:, v] = r["obs"]
    return ll.argmax(axis=1).astype(np.int32)


def flags(r, z_min, min_cells):
    """MISFIT per SNP: n_cell >= min_cells and Z < z_min."""
    z = zscore(r)
    with np.errstate(invalid="ignore"):
        return (r["n_cell"] >= min_cells) & (z < z_min)


def check_swapped_rounds(rounds, swapped, min_cells):
    """The four conditions of the swapped-rows pool on rounds[r] = (share of right singlets, flag[S], n_cell[S]), r = 0..3 (round 0
    carries no flags)."""
    share = [r[0] for r in rounds]
    last_flag, last_cells = rounds[-1][1], rounds[-1][2]
    assert not (last_flag & ~swapped).any(), int((last_flag & ~swapped).sum())
    seen = swapped & (last_cells >= min_cells)
    assert seen.sum() > 0.9 * swapped.sum()
    assert (seen & ~last_flag).sum() <= 0.02 * seen.sum(), (int((seen & ~last_flag).sum()), int(seen.sum()))
    assert share[1] > share[0], share
    for r in range(2, len(share)):
        assert share[r] >= share[r - 1], share
