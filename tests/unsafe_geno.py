"""Test-side genotype matrices that are NOT "safe" (k_check_geno: every row finite, non-negative, maximum >= 1e-30f), and the comparison
that goes with them.  An unsafe matrix runs the checked (CHK) kernels, whose flagged barcodes the fix-up pass recomputes with ocml's
log(); the results then hold -inf, +inf and NaN, which a plain |out - ref| < tol cannot compare.

poison() edits a handful of SNPs of a matrix.  The SNPs are the ones one barcode of the pileup covers at pair index 0, 31, 32 and last
(first / last pair of a walk, both sides of a 32-pair tile edge); the barcode is the one whose choice leaves the most OTHER barcodes
without any poisoned SNP (lowest id among equals), so that sparse pileups keep barcodes whose results must not move at all.
Every poisoned SNP gets ONE bad row (shared by the samples it is given to), so a GT matrix keeps <= 4 bitwise-distinct rows per SNP:
the class kernels stay selected, and a canonical GT matrix stays canonical with the bad row as the SNP's "other" row."""
import numpy as np

F32_EDGE = np.float32(1e-30)                       # k_check_geno's bound: a row whose maximum is exactly this is still safe
F32_BELOW = np.nextafter(F32_EDGE, np.float32(0))  # ... and this one is not
KINDS = ("zero", "nan", "edge_safe")


def covered_snps(sp, c):
    """SNP ids of barcode c's pairs, in stored order."""
    if sp.pair_snp is None:
        return np.arange(sp.n_snps, dtype=np.int64)
    return np.asarray(sp.pair_snp[sp.cell_pair_off[c]:sp.cell_pair_off[c + 1]], dtype=np.int64)


def covering(sp, snps):
    """bool [B]: the barcode covers at least one of the SNPs."""
    snps = np.asarray(list(snps), dtype=np.int64)
    return np.array([np.isin(covered_snps(sp, c), snps).any() for c in range(sp.n_cells)])


def target_snps(sp):
    """(barcode, [SNP at pair index 0, 31, 32, last]) — see the module docstring.  Needs a barcode of >= 34 pairs."""
    best = None
    for c in range(sp.n_cells):
        cs = covered_snps(sp, c)
        if len(cs) < 34:
            continue
        snps = [int(cs[0]), int(cs[31]), int(cs[32]), int(cs[-1])]
        clean = int((~covering(sp, snps)).sum())
        if best is None or clean > best[0]:
            best = (clean, c, snps)
    assert best is not None, "no barcode with 34 covered SNPs"
    return best[1], best[2]


def poison(g, kind, rng, sp, no_sample0=False, below=False):
    """A float32 copy of g [S][V][3] with the edits of `kind`, and the list of poisoned SNPs (in the order first, 31, 32, last).

    "zero"        all-zero rows: sample 0 (a random one with no_sample0) at the first SNP, sample V-1 at the last, one random sample at
                  the SNP of pair 31 and two at the SNP of pair 32.  Results: -inf, never NaN.
    "nan"         the SNP of pair 31 NaN for every sample (a GP record with a missing sample); one negative entry at the first SNP,
                  one +inf entry at the SNP of pair 32, the row (1e-45, 0, 0) — a float32 denormal: unsafe, finite results — at the last.
    "edge_safe"   the rows of "zero" scaled so that their maximum is exactly float32(1e-30): still safe, everything finite;
                  with `below`, the maximum is one float32 below 1e-30: unsafe by the check, harmless."""
    assert kind in KINDS
    g = np.array(g, dtype=np.float32, copy=True)
    S, V, _ = g.shape
    _, snps = target_snps(sp)
    s_first, s31, s32, s_last = snps
    mid = rng.choice(np.arange(1, V - 1), size=3, replace=False) if V >= 5 else rng.integers(0, V, size=3)
    first_sample = int(mid[2]) if no_sample0 else 0
    edits = [(s_first, [first_sample]), (s31, [int(mid[0])]), (s32, [int(mid[0]), int(mid[1])]), (s_last, [V - 1])]
    if kind == "zero":
        for s, ks in edits:
            g[s, ks] = 0.0
    elif kind == "nan":
        g[s31] = np.nan
        g[s_first, first_sample, 1] = np.float32(-1e-3)
        g[s32, int(mid[1]), 2] = np.inf
        g[s_last, V - 1] = (np.float32(1e-45), 0.0, 0.0)
    else:
        top = F32_BELOW if below else F32_EDGE
        for s, ks in edits:
            row = g[s, ks[0]].astype(np.float64)
            new = (row * (float(top) / row.max())).astype(np.float32)
            new[int(np.argmax(row))] = top
            assert new.max() == top
            g[s, ks] = new
    return g, snps


def is_safe(g):
    """k_check_geno on the host."""
    g = np.asarray(g, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        fin = ((g >= 0) & (g <= np.float32(3.0e38))).all(axis=-1)
        return bool((fin & (np.fmax.reduce(g, axis=-1) >= F32_EDGE)).all())


def assert_matches(out, ref, mask, tol, what=""):
    """Where ref is finite: |out - ref| < tol.  Where it is not: out has the same class at the same position (NaN <-> NaN, +inf <-> +inf,
    -inf <-> -inf).  Returns (finite entries compared, non-finite entries compared, largest finite |out - ref|)."""
    out, ref = np.asarray(out, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    mask = np.broadcast_to(np.ones((), dtype=bool) if mask is None else mask, ref.shape)
    o, r = out[mask], ref[mask]
    fin = np.isfinite(r)
    for name, cls in (("NaN", np.isnan), ("+inf", lambda x: np.isposinf(x)), ("-inf", lambda x: np.isneginf(x))):
        bad = np.flatnonzero(cls(r) != cls(o))
        assert bad.size == 0, f"{what}: {bad.size} entries differ in being {name}; first at {bad[0]}: out {o[bad[0]]!r} ref {r[bad[0]]!r}"
    with np.errstate(invalid="ignore"):
        d = np.abs(o[fin] - r[fin])
    worst = float(d.max()) if d.size else 0.0
    assert not (d >= tol).any(), f"{what}: max |out - ref| = {worst:.3e} over {int(fin.sum())} finite entries (tol {tol:g})"
    return int(fin.sum()), int((~fin).sum()), worst
