"""CPU: the goodness-of-fit model (tests/fit_ref.py, the restatement the GPU is compared with) and demuxlet_amd/fit.py's host side.

The restatement against a brute force that forms Pr(y) from per-read conditional probabilities; small-case identities; calibration on
pools drawn from the model; power on a pool with a donor dropped from the matrix; true doublets under their pair and under their first
donor alone; the command line, the `.best` row parsing and the TSV writers.

Calibration figures (seed 11, 400 barcodes, ~150 pairs each, gp softened by 0.3, M = 4), measured once: singlets mean -0.057, sd 0.966;
doublets mean +0.076, sd 1.037.  The bound on the mean is 3 / sqrt(n); the band of the sd is 1 +- 0.16: the sd of n = 400 unit normals
has a standard error of 1 / sqrt(2 (n - 1)) = 0.035, three of them are 0.106, widened by half."""
import itertools

import numpy as np
import pytest

import ambient_dbl_ref as AD
import ambient_ref as AR
import fit_ref as R


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import build, capi, engine, synth
    build.build()
    capi.load()
    mat, err = engine.phred_tables()
    return dict(engine=engine, synth=synth, mat=mat, err=err)


def gt_matrix(m, alleles):
    return np.stack([m["engine"].geno_from_gt(alleles[s], 0.01) for s in range(alleles.shape[0])])


def fit(m, sp, hyp, alpha, g, M, rho=None, a=None, **kw):
    return R.ref_fit(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, hyp, alpha, rho, a, g, M, m["mat"], m["err"], **kw)


def small_pool(m, seed, B=12, S=40, V=4, doublets=True):
    rng = np.random.default_rng(seed)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw.alleles)
    g[3, :] = np.array([1.0, 0.0, 0.0], dtype=np.float32)                       # hard zeros
    g[7, 1] = 0.0                                                               # an all-zero row
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.5, 2.0, doublet_rate=0.5 if doublets else 0.0, quals="edges")
    hyp = sp.truth.copy()
    hyp[B - 1] = (-1, -1)                                                       # an unused barcode
    alpha = np.where(hyp[:, 1] >= 0, rng.choice([0.0, 0.5, 0.37], size=B), 0.0)
    rho = rng.choice([0.0, 0.1, 0.3], size=B)
    a = rng.uniform(0.0, 1.0, size=S)
    return sp, g, hyp, alpha, rho, a


def brute_force_pair(m, rd, W, p):
    """(c0, mean of log L - c0, variance, Pr[2^n]) of one pair: Pr(y) = sum_c pi_c prod_r Pr(y_r | c), pi_c = W_c / sum W, with
    Pr(allele | c, the read is stored) = t_r(c, allele) / (t_r(c, 0) + t_r(c, 1)); log L(y) from the unnormalised factors."""
    mat, e3 = m["mat"], m["err"] / 3.0
    bq, x = rd & 127, rd >> 7
    t = np.stack([mat[bq][:, None] * (1 - p) + e3[bq][:, None] * p, e3[bq][:, None] * (1 - p) + mat[bq][:, None] * p], axis=2)    # [n][NC][2]
    cond = t / t.sum(axis=2, keepdims=True)
    pi = W / W.sum()
    pr, logL = [], []
    for y in itertools.product((0, 1), repeat=len(rd)):                         # y[0] = the first read's allele
        sel = np.array(y)
        pr.append(float((pi * np.prod(cond[np.arange(len(rd)), :, sel], axis=0)).sum()))
        logL.append(float(np.log((W * np.prod(t[np.arange(len(rd)), :, sel], axis=0)).sum())))
    pr, logL = np.array(pr), np.array(logL)
    code = [sum(b << r for r, b in enumerate(y)) for y in itertools.product((0, 1), repeat=len(rd))]
    order = np.argsort(code)
    pr, logL = pr[order], logL[order]
    c0 = logL[int(sum(int(b) << r for r, b in enumerate(x)))]
    e = float((pr * (logL - c0)).sum())
    return c0, e, float((pr * (logL - c0) ** 2).sum() - e * e), pr


def test_restatement_matches_brute_force(m):
    """Pr(y) = L(y) / sum L: the restatement's per-pair c0, mean and variance against per-read conditional probabilities."""
    sp, g, hyp, alpha, rho, a = small_pool(m, 3)
    M = 5
    r = fit(m, sp, hyp, alpha, g, M, rho, a, pairs=True)
    cell, snp, nrd, start, _ = R.host_pairs(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd)
    assert len(r["pairs"]) == r["n_snp"].sum() > 100
    kinds = set()
    for k, c0, e1, var, pr in r["pairs"]:
        b, i = cell[k], snp[k]
        v1, v2 = hyp[b]
        rd = np.asarray(sp.reads)[start[k]:start[k] + min(nrd[k], M)].astype(np.int64)
        if v2 < 0:
            W = g[i, v1].astype(np.float64)
            cm = np.array([0.0, 0.5, 1.0])
        else:
            W = np.array([float(g[i, v1, l]) * float(g[i, v2, k_]) for l in range(3) for k_ in range(3)])
            cm = AD.mix_constants(alpha[b])
        keep = W != 0                                                           # (a zero weight's component has no conditional law)
        p = (1 - rho[b]) * cm + rho[b] * a[i]
        bc0, be, bvar, bpr = brute_force_pair(m, rd, W[keep], p[keep])
        assert abs(c0 - bc0) <= 1e-12 * max(1.0, abs(bc0))
        assert abs(e1 - be) <= 1e-10 and abs(var - bvar) <= 1e-9 * max(1.0, bvar)
        assert np.allclose(pr, bpr, rtol=0, atol=1e-12)
        kinds.add((v2 >= 0, len(rd)))
    for dbl in (False, True):                                                   # both kinds, from one read to several
        assert (dbl, 1) in kinds and max(n for d_, n in kinds if d_ == dbl) >= 4


def test_small_case_identities(m):
    sp, g, hyp, alpha, rho, a = small_pool(m, 5)
    r = fit(m, sp, hyp, alpha, g, 4, rho, a, pairs=True)
    for _, _, _, var, pr in r["pairs"]:
        assert abs(pr.sum() - 1.0) <= 1e-14 and var >= 0.0
    assert (r["var"] >= 0).all() and r["n_trunc"].sum() > 0
    unused = hyp[:, 0] < 0
    for key in r:
        if key != "pairs":
            assert not np.asarray(r[key])[unused].any()
    # counts: pairs of used barcodes with a read and non-zero rows, reads capped at M
    cell, snp, nrd, _, _ = R.host_pairs(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd)
    ok = (hyp[cell, 0] >= 0) & (nrd > 0) & (g[snp, np.maximum(hyp[cell, 0], 0)] != 0).any(axis=1)
    ok &= (hyp[cell, 1] < 0) | (g[snp, np.maximum(hyp[cell, 1], 0)] != 0).any(axis=1)
    assert r["n_zero"].sum() == 0
    assert np.array_equal(r["n_snp"], np.bincount(cell[ok], minlength=sp.n_cells))
    assert np.array_equal(r["n_read"], np.bincount(cell[ok], weights=np.minimum(nrd, 4)[ok], minlength=sp.n_cells))
    assert np.array_equal(r["n_trunc"], np.bincount(cell[ok & (nrd > 4)], minlength=sp.n_cells))


def test_obs_is_the_ambient_profile_without_truncation(m):
    """With M >= every pair's depth, obs is dmx_engine_ambient's LL at (v1, rho) and dmx_engine_ambient_doublet's at (v1, v2, alpha, rho):
    against their restatements (which work in logs)."""
    sp, g, hyp, alpha, rho, a = small_pool(m, 7, B=24)
    nrd = np.asarray(sp.pair_nrd)
    assert 1 < nrd.max() <= 8
    r = fit(m, sp, hyp, alpha, g, 8, rho, a)
    assert r["n_trunc"].sum() == 0 and r["n_zero"].sum() == 0
    for b in range(sp.n_cells):
        v1, v2 = hyp[b]
        if v1 < 0:
            continue
        one = np.full(sp.n_cells, -1)
        one[b] = v1
        if v2 < 0:
            LL, ns, nr = AR.ref_profile(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, one, g, a, [rho[b]], m["mat"], m["err"])
            ll, ns, nr = LL[b, 0], ns[b], nr[b]
        else:
            cand = np.full((sp.n_cells, 1, 2), -1)
            cand[b, 0] = (v1, v2)
            LL, ns, nr = AD.ref_dbl_profile(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, cand, g, a, [alpha[b]], [rho[b]], m["mat"], m["err"])
            ll, ns, nr = LL[b, 0, 0, 0], ns[b, 0], nr[b, 0]
        assert ns == r["n_snp"][b] and nr == r["n_read"][b]
        assert abs(r["obs"][b] - ll) <= 1e-9 * max(1.0, abs(ll)), (b, r["obs"][b], ll)


def test_zero_likelihood_pairs_are_counted_apart(m):
    """A hard one-hot row contradicted by a read that cannot be wrong (tables with err = 0 at quality 0): L(x) = 0, the pair goes to n_zero
    and to none of the sums; the barcode's other pair, contradicted at quality 30, still counts."""
    synth = m["synth"]
    g = np.zeros((2, 2, 3), dtype=np.float32)
    g[:, :, 0] = 1.0                                                            # hom-REF, hard
    mat, err = m["mat"].copy(), m["err"].copy()
    mat[0], err[0] = 1.0, 0.0                                                   # tables under which a quality-0 read cannot be wrong
    reads = np.array([(1 << 7) | 0, 30, (1 << 7) | 30], dtype=np.uint8)         # SNP 0: ALT at q0 (impossible), REF; SNP 1: ALT at q30
    t = np.ones(1, dtype=np.int32)
    sp = synth.SynthPileup(1, 2, np.array([0, 2]), np.array([0, 3]), np.array([0, 1], dtype=np.int32), np.array([2, 1], dtype=np.uint8), reads,
                           t, t, t, np.array([[0, -1]], dtype=np.int32))
    r = R.ref_fit(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, [[0, -1]], [0.0], None, None, g, 4, mat, err)
    assert r["n_zero"][0] == 1 and r["n_snp"][0] == 1 and r["n_read"][0] == 1
    assert np.isfinite(r["obs"][0]) and r["obs"][0] < -5.0


def calibration(m, seed, doublets):
    rng = np.random.default_rng(seed)
    S, V, B = 3000, 4, 400
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = np.stack([m["engine"].geno_from_gp(x, 0.01) for x in m["synth"].raw_gp_from_alleles(rng, raw.alleles, soft=0.3)])
    v1 = np.arange(B) % V
    hyp = np.stack([v1, (v1 + 1) % V if doublets else np.full(B, -1)], axis=1).astype(np.int32)
    alpha = np.full(B, 0.5 if doublets else 0.0)
    sp = R.model_drawn_pool(rng, m["synth"], g, B, 0.05, 1.5, hyp, alpha, M=4)
    z = R.zscore(fit(m, sp, hyp, alpha, g, 4))
    return z, float(np.diff(sp.cell_pair_off).mean())


@pytest.mark.parametrize("doublets", [False, True])
def test_calibration_on_model_drawn_pools(m, doublets):
    z, pairs = calibration(m, 11 + doublets, doublets)
    n = len(z)
    print(f"calibration doublets={doublets}: n {n} pairs/barcode {pairs:.0f} mean {z.mean():+.4f} sd {z.std(ddof=1):.4f}")
    assert np.isfinite(z).all() and 120 < pairs < 180
    assert abs(z.mean()) <= 3.0 / np.sqrt(n), z.mean()
    assert 0.84 <= z.std(ddof=1) <= 1.16, z.std(ddof=1)


def power_pool(m):
    """8 donors, donor 0 missing from the matrix, 160 singlets of ~150 covered SNPs at 1.25 reads: chosen on the CPU so that the restatement
    alone separates the two groups (see DESIGN.md section 26 for the figures)."""
    rng = np.random.default_rng(7)
    sp, g, truth = R.dropped_donor_pool(rng, m["synth"], lambda al: m["engine"].geno_from_gt(al, 0.01), 1500, 8, 160, 0.1, 1.25)
    hyp = R.dropped_donor_hypotheses(sp, g, truth, m["mat"], m["err"])
    return sp, g, truth, hyp


def test_power_on_a_dropped_donor_pool(m):
    sp, g, truth, hyp = power_pool(m)
    z = R.zscore(fit(m, sp, hyp, np.zeros(sp.n_cells), g, 4))
    right, missing = z[truth >= 0], z[truth < 0]
    print(f"power: correct barcodes z {right.min():+.2f} .. {right.max():+.2f}; the dropped donor's cells z <= {missing.max():+.2f}")
    assert len(right) == 140 and len(missing) == 20
    assert (right > -3.0).all(), right.min()
    assert (missing < -4.0).all(), missing.max()


def test_doublets_under_two_hypotheses(m):
    """True doublets fit under their true pair and misfit under their first donor alone."""
    rng = np.random.default_rng(5)
    S, V, B = 2000, 6, 120
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw.alleles)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.1, 1.5, doublet_rate=1.0)
    assert (sp.truth[:, 1] >= 0).all()
    alpha = np.full(B, 0.5)
    zd = R.zscore(fit(m, sp, sp.truth, alpha, g, 4))
    sng = np.stack([sp.truth[:, 0], np.full(B, -1)], axis=1)
    zs = R.zscore(fit(m, sp, sng, alpha, g, 4))
    print(f"doublets: under the pair z {zd.min():+.2f} .. {zd.max():+.2f}; under the first donor z {zs.min():+.2f} .. {zs.max():+.2f}")
    assert (zd > -3.0).all(), zd.min()
    assert (zs < -4.0).all(), zs.max()


def test_longdouble_switch_sizes_the_drift(m):
    sp, g, hyp, alpha, rho, a = small_pool(m, 9, B=40, S=200)
    r64 = fit(m, sp, hyp, alpha, g, 8, rho, a)
    rld = fit(m, sp, hyp, alpha, g, 8, rho, a, longdouble=True)
    assert rld["obs"].dtype == np.longdouble and r64["obs"].dtype == np.float64
    for k in ("n_snp", "n_read", "n_trunc", "n_zero"):
        assert np.array_equal(r64[k], rld[k])
    d = R.drift(r64, rld)
    print(f"float64 against longdouble drift {d:.3g}")
    assert d <= 1e-12
    assert R.tolerance(r64, rld) == 1e-9


# ---- demuxlet_amd/fit.py: parsing, rows, writers ---------------------------------------------------------------------------------------

BEST_HEAD = ("BARCODE\tRD.TOTL\tRD.PASS\tRD.UNIQ\tN.SNP\tBEST\tSNG.1ST\tSNG.LLK1\tSNG.2ND\tSNG.LLK2\tSNG.LLK0\tDBL.1ST\tDBL.2ND\tALPHA\tLLK12\tLLK1\tLLK2\t"
             "LLK10\tLLK20\tLLK00\tPRB.DBL\tPRB.SNG1\n")


def best_row(bc, best, s1, l1, s2, d1, d2, alpha, l12):
    return f"{bc}\t9\t9\t9\t5\t{best}\t{s1}\t{l1}\t{s2}\t-9.0\t-9.5\t{d1}\t{d2}\t{alpha}\t{l12}\t-1\t-1\t-1\t-1\t-1\t0.1\t0.9\n"


def test_command_line_parsing():
    from demuxlet_amd import fit as F
    a = F.parse_args(["--pileup", "x.txt", "--out", "o"])
    assert a.max_reads == 4 and a.z_min == -4.0 and a.best is None and a.ambient == "reads" and a.ambient_tsv is None and a.alpha == [0.0, 0.5]
    a = F.parse_args(["--pileup", "x.txt", "--out", "o", "--best", "b", "--max-reads", "8", "--z-min", "-3", "--ambient-tsv", "t", "--ambient", "census",
                      "--alpha", "0", "0.25", "--fast", "--gpu", "1"])
    assert (a.best, a.max_reads, a.z_min, a.ambient_tsv, a.ambient, a.alpha, a.fast, a.gpu) == ("b", 8, -3.0, "t", "census", [0.0, 0.25], True, 1)
    for bad in (["--out", "o"], ["--pileup", "x", "--out", "o", "--max-reads", "0"], ["--pileup", "x", "--out", "o", "--max-reads", "9"],
                ["--pileup", "x", "--out", "o", "--z-min", "nan"], ["--pileup", "x", "--out", "o", "--ambient", "reads"]):
        with pytest.raises(SystemExit):
            F.parse_args(bad)


def test_best_rows_become_hypotheses(tmp_path):
    from demuxlet_amd import fit as F
    samples = ["S-0", "S-1", "S-2"]
    barcodes = ["AAA-1", "CCC-1", "GGG-1", "TTT-1", "NNN-1", "ACG-1"]
    p = tmp_path / "x.best"
    p.write_text(BEST_HEAD
                 + best_row("AAA-1", "SNG-S-1", "S-1", -10.0, "S-0", "S-1", "S-2", 0.5, -12.0)
                 + best_row("CCC-1", "DBL-S-0-S-2-0.500", "S-0", -30.0, "S-2", "S-0", "S-2", 0.5, -20.0)
                 + best_row("GGG-1", "AMB-S-2-S-0-S-2/S-1", "S-2", -10.0, "S-0", "S-2", "S-1", 0.25, -9.0)      # the doublet's LLK is higher
                 + best_row("TTT-1", "AMB-S-2-S-0-S-2/S-1", "S-2", -10.0, "S-0", "S-2", "S-1", 0.25, -10.0)     # a tie: the singlet
                 + best_row("ACG-1", "DBL-S-1-S-1-0.500", "S-1", -10.0, "S-0", "S-1", "S-1", 0.5, -9.0))        # no pair: the singlet
    r = F.read_best_hypotheses(str(p), samples, barcodes)
    assert r.hyp.tolist() == [[1, -1], [0, 2], [2, 1], [2, -1], [-1, -1], [1, -1]]
    assert r.alpha.tolist() == [0.0, 0.5, 0.25, 0.0, 0.0, 0.0]
    assert r.has_row.tolist() == [True, True, True, True, False, True] and r.sng1.tolist() == [1, 0, 2, 2, -1, 1]
    assert F.hypothesis_label(0, 2, 0.5, samples) == "DBL-S-0-S-2-0.500" and F.hypothesis_label(1, -1, 0.0, samples) == "SNG-S-1"
    (tmp_path / "bad.best").write_text(BEST_HEAD + best_row("ZZZ-1", "SNG-S-1", "S-1", -1, "S-0", "S-1", "S-2", 0.5, -2))
    with pytest.raises(ValueError, match="barcode"):
        F.read_best_hypotheses(str(tmp_path / "bad.best"), samples, barcodes)
    (tmp_path / "bad2.best").write_text(BEST_HEAD + best_row("AAA-1", "SNG-S-9", "S-9", -1, "S-0", "S-1", "S-2", 0.5, -2))
    with pytest.raises(ValueError, match="sample"):
        F.read_best_hypotheses(str(tmp_path / "bad2.best"), samples, barcodes)
    (tmp_path / "bad3.best").write_text("BARCODE\tBEST\n")
    with pytest.raises(ValueError, match="column"):
        F.read_best_hypotheses(str(tmp_path / "bad3.best"), samples, barcodes)
    (tmp_path / "bad4.best").write_text(BEST_HEAD + best_row("AAA-1", "XYZ-S-1", "S-1", -1, "S-0", "S-1", "S-2", 0.5, -2))
    with pytest.raises(ValueError, match="BEST"):
        F.read_best_hypotheses(str(tmp_path / "bad4.best"), samples, barcodes)


def test_fit_writers(tmp_path):
    from demuxlet_amd import fit as F
    samples = ["S-0", "S-1"]
    barcodes = ["TTT-1", "AAA-1", "CCC-1", "GGG-1"]
    rows = F.BestHyp(["SNG-S-0", "SNG-S-0", "DBL-S-0-S-1-0.500", ""], np.array([[0, -1], [0, -1], [0, 1], [-1, -1]], dtype=np.int32),
                     np.array([0.0, 0.0, 0.5, 0.0]), np.array([0, 0, 0, -1], dtype=np.int32))
    r = dict(obs=np.array([-10.0, -30.0, -12.0, 0.0]), mean=np.array([-11.0, -10.0, -12.0, 0.0]), var=np.array([4.0, 4.0, 0.0, 0.0]),
             n_snp=np.array([5, 6, 7, 0]), n_read=np.array([6, 7, 9, 0]), n_trunc=np.array([0, 1, 0, 0]), n_zero=np.array([0, 0, 1, 0]))
    z = F.z_scores(r["obs"], r["mean"], r["var"])
    assert z[:2].tolist() == [0.5, -10.0] and np.isnan(z[2:]).all()
    p = F.lower_tail(z)
    assert abs(p[0] - 0.6914624612740131) < 1e-15 and p[1] < 1e-22 and np.isnan(p[2])
    z1 = np.array([0.5, -10.0, -7.0, np.nan])
    n = F.write_fit_tsv(str(tmp_path / "o.fit.tsv"), barcodes, samples, rows, r, z, p, z1, -4.0)
    lines = (tmp_path / "o.fit.tsv").read_text().splitlines()
    assert n == 1 and lines[0] == F.FIT_HEADER.rstrip("\n") and len(lines) == 4
    assert [l.split("\t")[0] for l in lines[1:]] == ["AAA-1", "CCC-1", "TTT-1"]          # byte-wise barcode order, no row for GGG-1
    assert lines[1].split("\t") == ["AAA-1", "SNG-S-0", "SNG-S-0", "6", "7", "1", "0", "-30.00000", "-10.00000", "2.00000", "-10.0000",
                                    lines[1].split("\t")[11], "-10.0000", "MISFIT"]
    assert lines[2].split("\t")[2:] == ["DBL-S-0-S-1-0.500", "7", "9", "0", "1", "-12.00000", "-12.00000", "0.00000", "NA", "NA", "-7.0000", "."]
    assert lines[3].split("\t")[-1] == "." and lines[3].split("\t")[10] == "0.5000"
    s = F.donor_summary(rows, z, -4.0, 2)
    assert s[0] == (0, 2, -4.75, -10.0, 1) and s[1][:2] == (1, 0) and np.isnan(s[1][2]) and s[2][:2] == (2, 1) and s[3][:2] == (3, 3) and s[3][4] == 1
    F.write_donors_tsv(str(tmp_path / "o.fit_donors.tsv"), samples, s)
    d = (tmp_path / "o.fit_donors.tsv").read_text().splitlines()
    assert d[0] == F.DONORS_HEADER.rstrip("\n") and len(d) == 5
    assert d[1] == "S-0\t2\t-4.7500\t-10.0000\t1\t0.5000" and d[2] == "S-1\t0\tNA\tNA\t0\tNA" and d[3].startswith("DBL\t1\tNA") and d[4].startswith("#POOL\t3\t")
    (tmp_path / "a.tsv").write_text("BARCODE\tSM_ID\tRHO\nAAA-1\tS-0\t0.1200\n")
    assert F.read_rho_tsv(str(tmp_path / "a.tsv"), barcodes).tolist() == [0.0, 0.12, 0.0, 0.0]
    (tmp_path / "b.tsv").write_text("BARCODE\tSM_ID\tRHO\nQQQ-1\tS-0\t0.1200\n")
    with pytest.raises(ValueError):
        F.read_rho_tsv(str(tmp_path / "b.tsv"), barcodes)


def test_struct_mirrors_match_the_c_compiler(tmp_path):
    import ctypes as C
    import subprocess
    from pathlib import Path
    from demuxlet_amd import capi
    root = Path(__file__).resolve().parents[1]
    (tmp_path / "s.c").write_text('#include "dmx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", '
                                  'sizeof(dmx_fit_request), offsetof(dmx_fit_request, hyp), offsetof(dmx_fit_request, ambient), sizeof(dmx_fit_info), '
                                  'offsetof(dmx_fit_info, n_zero), offsetof(dmx_fit_info, max_reads));return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{root / 'include'}", str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = list(map(int, subprocess.check_output([str(tmp_path / "s")], text=True).split()))
    assert got == [C.sizeof(capi.FitRequest), capi.FitRequest.hyp.offset, capi.FitRequest.ambient.offset, C.sizeof(capi.FitInfo),
                   capi.FitInfo.n_zero.offset, capi.FitInfo.max_reads.offset]
