"""numpy restatement of the anchored doublet search's contract (include/dmx.h) over ONE barcode's full grid
llksAB[V][V][A] and llks00[A]: the anchors, the evaluated set D_b and the record.  Test-side code: plain loops in the reference's
scan orders (cmd_cram_demuxlet.cpp:713-734, :746-758, :799-828), no attempt at speed."""
import numpy as np

TOL = 1e-7
NEAR_DOUBLET, NEAR_SINGLET, NEAR_RULE = 1, 2, 16


def choose_anchors(sing, T):
    """T times the first maximum of sing[] in ascending j among the samples not yet chosen (strict <); -1 when nothing compares."""
    out = []
    for _ in range(T):
        best, mx = -1, -1e300
        for j, v in enumerate(sing):
            if j in out:
                continue
            if mx < v:
                best, mx = j, v
        out.append(best)
    return np.array(out, dtype=np.int32)


def mask_db(V, A, anchors):
    """D_b = {(j, k, n) : n >= 1, j != k, and (j is an anchor, or k is an anchor, or k = 0)} as a boolean [V][V][A]."""
    m = np.zeros((V, V, A), dtype=bool)
    m[:, 0, 1:] = True
    for a in anchors:
        if a >= 0:
            m[a, :, 1:] = True
            m[:, a, 1:] = True
    for j in range(V):
        m[j, j, :] = False
    return m


def pairs_from_grid(grid, anchors):
    """pairs[t][k][0][n-1] = grid[a_t][k][n], pairs[t][k][1][n-1] = grid[k][a_t][n]; 0 at k = a_t and in the rows of unused anchors."""
    V, _, A = grid.shape
    p = np.zeros((len(anchors), V, 2, A - 1))
    for t, a in enumerate(anchors):
        if a < 0:
            continue
        p[t, :, 0, :] = grid[a, :, 1:]
        p[t, :, 1, :] = grid[:, a, 1:]
        p[t, a] = 0.0
    return p


def record(grid, l00, alphas, prior, n_pairs, summary_dtype, anchors=None, T=2):
    """(anchors, record) of one barcode.  `anchors`: explicit ids (-1 = unused), or None = choose T on the grid's own singlet column.
    A barcode without pairs gets K3's record of its (all-zero) grid."""
    V, _, A = grid.shape
    sing = grid[:, 0, 0]
    anc = choose_anchors(sing, T) if anchors is None else np.asarray(anchors, dtype=np.int32)
    s = np.zeros((), dtype=summary_dtype)
    m = mask_db(V, A, anc) if n_pairs > 0 else mask_db(V, A, range(V))
    mx = -1e300
    for v in sing:
        if mx < v: mx = v
    for v in grid[m]:
        if mx < v: mx = v
    ss = 0.0; sd = 0.0
    for j in range(V):
        ss += (np.exp(sing[j] - mx) * (1. - prior) / V)
    for j, k, n in zip(*np.nonzero(m)):
        sd += (np.exp(grid[j, k, n] - mx) * prior / V / (V - 1) / (A - 1) / (2.0 if alphas[n] == 0.5 else 1.0))
    i1 = i2 = -1; m1 = m2 = -1e300
    for j in range(V):
        v = sing[j]
        if m1 < v: m2, i2, i1, m1 = m1, i1, j, v
        elif m2 < v: i2, m2 = j, v
    jb = kb = nb = -1; mab = -1e300
    for j, k, n in zip(*np.nonzero(m)):                # np.nonzero walks (j, k, n) in row-major = the reference's scan order
        if mab < grid[j, k, n]: jb, kb, nb, mab = j, k, n, grid[j, k, n]
    s["max_llk"], s["sum_single"], s["sum_double"] = mx, ss, sd
    s["i_sing1"], s["i_sing2"], s["j_best"], s["k_best"], s["n_best"] = i1, i2, jb, kb, nb
    s["sing_llk1"], s["sing_llk2"] = sing[i1], sing[i2]
    s["llk12"], s["llk1"], s["llk2"] = grid[jb, kb, nb], sing[jb], sing[kb]
    s["llk10"], s["llk20"] = grid[jb, 0, nb], grid[kb, 0, nb]
    s["llk00_0"], s["llk00_best"] = l00[0], l00[nb]
    s["n_pairs"] = n_pairs
    # k_reduce's near-tie flags over the evaluated entries
    flags = 0
    mirror = (kb, jb, nb) if alphas[nb] == 0.5 else None
    for j, k, n in zip(*np.nonzero(m)):
        if (j, k, n) != (jb, kb, nb) and (j, k, n) != mirror and grid[j, k, n] >= mab - TOL:
            flags |= NEAR_DOUBLET
            break
    if i2 >= 0 and (int(np.sum(sing >= m2 - TOL)) > 2 or m1 - m2 < TOL):
        flags |= NEAR_SINGLET
    l12, l1, l2 = grid[jb, kb, nb], sing[jb], sing[kb]
    if i2 >= 0 and (abs(l12 - (m1 + 2)) < TOL or abs(m1 - (m2 + 2)) < TOL or
                    ((abs(l12 - l1) < TOL or abs(l12 - l2) < TOL) and l12 > m1 + 2 - TOL)):
        flags |= NEAR_RULE
    s["flags"] = flags
    return anc, s


def best_entry(grid):
    """(j, k, n) of the full grid's best doublet entry: the first maximum over j != k, n >= 1 in the reference's scan order (:799-814)."""
    V, _, A = grid.shape
    jb = kb = nb = -1; mab = -1e300
    for j in range(V):
        for k in range(V):
            if j == k: continue
            for n in range(1, A):
                if mab < grid[j, k, n]: jb, kb, nb, mab = j, k, n, grid[j, k, n]
    return jb, kb, nb


def missed(grid, alphas, anchors):
    """Whether the full grid's best doublet entry (j, k, n) lies outside D_b.  At alpha[n] = 0.5 the mirror (k, j, n) is the same hypothesis
    (the arbiter settles the order) and counts as well; at any other alpha it is another entry and does not."""
    V, _, A = grid.shape
    jb, kb, nb = best_entry(grid)
    m = mask_db(V, A, anchors)
    return not (m[jb, kb, nb] or (alphas[nb] == 0.5 and m[kb, jb, nb]))


def donor_among(grid, anchors):
    """Whether a donor of the full grid's best pair is one of `anchors`."""
    jb, kb, _ = best_entry(grid)
    return jb in list(anchors) or kb in list(anchors)


INDEX_FIELDS = ("i_sing1", "i_sing2", "j_best", "k_best", "n_best", "n_pairs")
LLK_FIELDS = ("sing_llk1", "sing_llk2", "llk12", "llk1", "llk2", "llk10", "llk20", "llk00_0", "llk00_best")


def ratios(s):
    """The two printed ratios in which max_llk cancels: PRB.DBL and PRB.SNG1."""
    return (float(s["sum_double"] / (s["sum_single"] + s["sum_double"])), float(np.exp(s["sing_llk1"] - s["max_llk"]) / s["sum_single"]))


# The pools of the end-to-end test: (seed, B, S, V, delta, alphas, soft).  rng = default_rng(seed), make_raw_genotypes, (soft: raw_gp_from_alleles
# drawn between the two calls,) make_pileup at 1.25 reads per pair with 30 % doublets; GT error 0.01.
E2E_POOLS = [(3, 60, 2000, 40, 0.1, (0.0, 0.5), False), (11, 48, 1200, 100, 0.1, (0.0, 0.5), False), (13, 64, 1500, 24, 0.1, (0.0, 0.25, 0.5), False),
             (12, 96, 2000, 24, 0.08, (0.0, 0.5), True)]
LOW_DEPTH_POOL = (205, 200, 3000, 16, 0.01)


def e2e_pool(synth, conv, seed, B, S, V, delta, soft=False):
    """(pileup, genotype matrix); `conv` has geno_from_gt / geno_from_gp (the engine module or the oracle's)."""
    rng = np.random.default_rng(seed)
    raw = synth.make_raw_genotypes(rng, S, V)
    gp = synth.raw_gp_from_alleles(rng, raw.alleles) if soft else None
    sp = synth.make_pileup(rng, raw.alleles, B, delta, 1.25, doublet_rate=0.3)
    if soft:
        g = np.stack([conv.geno_from_gp(x, 0.01) for x in gp])
    else:
        g = np.stack([conv.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    return sp, g
