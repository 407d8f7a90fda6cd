"""CPU: the host side of the ambient-aware doublet profile (demuxlet_amd/ambient.py: `.best` reader, candidate builder, decision rule,
writer, command-line argument errors; synth.make_ambient_mixed_pileup) and the numpy restatement (tests/ambient_dbl_ref.py) against an
mpmath per-read product and against the singlet restatement at alpha = 0.  No GPU compute is called."""
import numpy as np
import pytest

import ambient_dbl_ref as D
import ambient_ref as R


@pytest.fixture(scope="module")
def mods():
    from demuxlet_amd import ambient, build, capi, engine, synth
    build.build()
    capi.load()
    return dict(ambient=ambient, capi=capi, engine=engine, synth=synth)


def one_cell(pairs, S):
    """A one-barcode CSR pileup from [(snp, read bytes)]."""
    po = np.array([0, len(pairs)], dtype=np.int64)
    return po, np.array([s for s, _ in pairs], dtype=np.int32), np.array([len(r) for _, r in pairs], dtype=np.int64), \
        np.concatenate([np.asarray(r, dtype=np.uint8) for _, r in pairs] + [np.zeros(0, dtype=np.uint8)])


def mp_profile(pairs, g, v1, v2, a, alpha, rho, mat, err):
    """200-bit: sum over pairs of log(sum_lm gp1_l gp2_m prod over reads (pR (1 - p) + pA p))."""
    import mpmath as mp
    mp.mp.prec = 200
    tot = mp.mpf(0)
    for snp, rd in pairs:
        g1, g2 = g[snp, v1], g[snp, v2]
        if len(rd) == 0 or not g1.any() or not g2.any():
            continue
        L = mp.mpf(0)
        for l in range(3):
            for m in range(3):
                p = (1 - mp.mpf(rho)) * (mp.mpf(0.5) * l + (m - l) * mp.mpf(0.5) * mp.mpf(alpha)) + mp.mpf(rho) * mp.mpf(float(a[snp]))
                f = mp.mpf(1)
                for b in rd:
                    bq, alt = int(b) & 127, int(b) >> 7
                    pR = mp.mpf(float(err[bq])) / 3 if alt else mp.mpf(float(mat[bq]))
                    pA = mp.mpf(float(mat[bq])) if alt else mp.mpf(float(err[bq])) / 3
                    f *= pR * (1 - p) + pA * p
                L += mp.mpf(float(g1[l])) * mp.mpf(float(g2[m])) * f
        tot += mp.log(L)
    return float(tot)


def test_restatement_against_mpmath(mods):
    """Small soft rows and a 400-read ALT-heavy pair on hom-REF x hom-REF hard rows, whose float64 product underflows."""
    mat, err = mods["engine"].phred_tables()
    rng = np.random.default_rng(3)
    S, V = 12, 3
    g = rng.dirichlet([1, 1, 1], size=(S, V)).astype(np.float32)
    g[5, :] = np.array([1.0, 0.0, 0.0], dtype=np.float32)
    g[7, 1] = 0.0                                   # all-zero row: the pair is skipped for candidates that use sample 1
    deep = np.where(rng.random(400) < 0.9, (1 << 7) | 40, 35).astype(np.uint8)
    pairs = [(1, [30, (1 << 7) | 20]), (3, [(1 << 7) | 0]), (5, deep), (7, [40, 40, (1 << 7) | 127]), (9, []), (10, [1, (1 << 7) | 127, 127])]
    assert np.prod([float(err[40]) / 3] * 360) == 0.0
    po, snp, nrd, reads = one_cell(pairs, S)
    a = rng.uniform(0.05, 0.95, size=S)
    alphas, grid = [0.0, 0.3, 0.5, 1.0], [0.0, 0.01, 0.2, 1.0]
    cand = np.array([[[0, 1], [2, 0], [-1, -1], [1, 2]]], dtype=np.int32)
    LL, ns, nr = D.ref_dbl_profile(po, snp, nrd, reads, cand, g, a, alphas, grid, mat, err)
    assert ns[0].tolist() == [4, 5, 0, 4] and nr[0, 1] == 2 + 1 + 400 + 3 + 3 and nr[0, 0] == nr[0, 1] - 3
    assert not LL[0, 2].any() and np.isfinite(LL).all()
    assert LL[0, 1, 0, 0] < -2000                   # the deep pair at alpha = 0, rho = 0
    for c in (0, 1, 3):
        for ai, al in enumerate(alphas):
            for qi, rho in enumerate(grid):
                x = mp_profile(pairs, g, int(cand[0, c, 0]), int(cand[0, c, 1]), a, al, rho, mat, err)
                assert abs(LL[0, c, ai, qi] - x) <= 1e-10 * max(1.0, abs(x) * 1e-2), (c, al, rho, LL[0, c, ai, qi], x)


def test_alpha_zero_is_the_singlet_restatement(mods):
    """alpha = 0 and exactly one-hot rows for v2: the doublet restatement equals ambient_ref.ref_profile for assign = v1."""
    synth, eng = mods["synth"], mods["engine"]
    mat, err = eng.phred_tables()
    rng = np.random.default_rng(5)
    S, V, B = 300, 4, 30
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    g[:, 3] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, size=S)]
    sp, _, _, a = synth.make_ambient_mixed_pileup(rng, raw.alleles, B, 0.2, 1.5, 0.2, False)
    v1 = (np.arange(B) % 3).astype(np.int32)
    cand = np.stack([v1, np.full(B, 3, dtype=np.int32)], axis=1)[:, None, :]
    grid = np.linspace(0, 1, 11)
    LL, ns, nr = D.ref_dbl_profile(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, cand, g, a, [0.0], grid, mat, err)
    L1, n1, r1 = R.ref_profile(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, v1, g, a, grid, mat, err)
    assert np.array_equal(ns[:, 0], n1) and np.array_equal(nr[:, 0], r1)
    assert np.abs(LL[:, 0, 0, :] - L1).max() <= 1e-12


def test_symmetry_of_the_restatement(mods):
    synth, eng = mods["synth"], mods["engine"]
    mat, err = eng.phred_tables()
    rng = np.random.default_rng(6)
    S, V, B = 200, 4, 12
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    sp, _, _, a = synth.make_ambient_mixed_pileup(rng, raw.alleles, B, 0.3, 1.5, 0.1, True, 0.3)
    c1 = np.tile(np.array([[[0, 2]]], dtype=np.int32), (B, 1, 1))
    c2 = c1[:, :, ::-1].copy()
    grid = [0.0, 0.1, 0.5]
    x, _, _ = D.ref_dbl_profile(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, c1, g, a, [0.25, 0.5], grid, mat, err)
    y, _, _ = D.ref_dbl_profile(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads, c2, g, a, [0.5, 0.75], grid, mat, err)
    assert np.abs(x[:, 0, 0] - y[:, 0, 1]).max() <= 1e-10 and np.abs(x[:, 0, 1] - y[:, 0, 0]).max() <= 1e-10


BEST_HEAD = "BARCODE\tRD.TOTL\tRD.PASS\tRD.UNIQ\tN.SNP\tBEST\tSNG.1ST\tSNG.LLK1\tSNG.2ND\tSNG.LLK2\tSNG.LLK0\tDBL.1ST\tDBL.2ND\tALPHA\tLLK12\tLLK1\tLLK2\tLLK10\tLLK20\tLLK00\tPRB.DBL\tPRB.SNG1\n"


def best_row(bc, best, s1, s2, d1, d2):
    return f"{bc}\t9\t9\t9\t5\t{best}\t{s1}\t-1.0\t{s2}\t-2.0\t-3.0\t{d1}\t{d2}\t0.500\t-1\t-1\t-1\t-1\t-1\t-1\t0.5\t0.5\n"


def test_best_reader_and_candidates(mods, tmp_path):
    A = mods["ambient"]
    samples = ["S-0", "S-1", "S-2", "S-3"]
    barcodes = ["bc0", "bc1", "bc2", "bc3", "bc4"]
    p = tmp_path / "x.best"
    p.write_text(BEST_HEAD
                 + best_row("bc3", "DBL-S-0-S-1-0.500", "S-0", "S-1", "S-1", "S-0")       # same unordered pair: one candidate
                 + best_row("bc0", "SNG-S-2", "S-2", "S-3", "S-2", "S-0")                 # two candidates
                 + best_row("bc1", "AMB-S-1-S-0-S-1/S-3", "S-1", "S-0", "S-1", "S-3")
                 + best_row("bc4", "DBL-S-3-S-3-0.500", "S-1", "S-2", "S-3", "S-3"))      # a degenerate doublet pair is not used
    rows = A.read_best_rows(str(p), samples, barcodes)
    assert rows.best == ["SNG-S-2", "AMB-S-1-S-0-S-1/S-3", "", "DBL-S-0-S-1-0.500", "DBL-S-3-S-3-0.500"]
    assert rows.sng1.tolist() == [2, 1, -1, 0, 1] and rows.sng2.tolist() == [3, 0, -1, 1, 2]
    assert rows.dbl1.tolist() == [2, 1, -1, 1, 3] and rows.dbl2.tolist() == [0, 3, -1, 0, 3]
    assert rows.has_row.tolist() == [True, True, False, True, True]
    cand = A.candidates_from_best(rows)
    assert cand.shape == (5, 2, 2) and cand.dtype == np.int32
    assert cand.tolist() == [[[2, 0], [2, 3]], [[1, 3], [1, 0]], [[-1, -1], [-1, -1]], [[1, 0], [-1, -1]], [[-1, -1], [1, 2]]]
    with pytest.raises(ValueError):
        A.read_best_rows(str(p), samples[:3], barcodes)
    with pytest.raises(ValueError):
        A.read_best_rows(str(p), samples, barcodes[:3])
    q = tmp_path / "y.best"
    q.write_text("BARCODE\tBEST\n")
    with pytest.raises(ValueError):
        A.read_best_rows(str(q), samples, barcodes)


def test_decision_rule_at_its_thresholds(mods):
    A = mods["ambient"]
    s1 = np.array([-100.0] * 8)
    s2 = np.array([-102.0, -102.0, -102.5, -102.5, -102.0, -90.0, -np.inf, -102.0 - 1e-9])
    d = np.array([-98.0, -98.0 + 1e-9, -98.0, -97.0, -np.inf, -98.0, -np.inf, -98.0])
    got = A.decide(s1, s2, d).tolist()
    # DBL needs LLK.DBL > LLK.SNG1 + 2 (a tie is not enough); SNG needs LLK.SNG1 > LLK.SNG2 + 2 (same); everything else is AMB
    assert got == [A.CALL_AMB, A.CALL_DBL, A.CALL_SNG, A.CALL_DBL, A.CALL_AMB, A.CALL_AMB, A.CALL_SNG, A.CALL_SNG]
    assert A.CALL_MARGIN == 2.0


def test_make_calls_and_writer(mods, tmp_path):
    A = mods["ambient"]
    samples = ["a", "b-1", "c"]
    barcodes = ["T-1", "A-1", "C-1", "G-1"]
    rows = A.BestRows(["SNG-a", "DBL-a-c-0.500", "", "SNG-c"], np.array([0, 0, -1, 2], dtype=np.int32), np.array([1, 2, -1, 1], dtype=np.int32),
                      np.array([0, 0, -1, 2], dtype=np.int32), np.array([2, 2, -1, 0], dtype=np.int32))
    cand = A.candidates_from_best(rows)
    assert cand.tolist() == [[[0, 2], [0, 1]], [[0, 2], [-1, -1]], [[-1, -1], [-1, -1]], [[2, 0], [2, 1]]]
    grid = np.array([0.0, 0.1, 0.2])
    al = np.array([0.25, 0.5])
    ll1 = np.array([[-10.0, -8.0, -8.0], [-30.0, -31.0, -32.0], [0, 0, 0], [-5.0, -5.5, -6.0]])
    ll2 = np.array([[-20.0, -19.0, -18.0], [-30.5, -31.0, -32.0], [0, 0, 0], [-6.0, -7.0, -8.0]])
    lld = np.full((4, 2, 2, 3), -50.0)
    lld[0, 1, 1, 2] = -7.0                     # below LLK.SNG1 + 2 = -6: stays a singlet
    lld[0, 0, 0, 1] = -7.0                     # a tie: the lowest (candidate, alpha, rho) index is reported
    lld[1, 0, 1, 0] = -20.0                    # DBL
    lld[1, 1] = 0.0                            # an unused slot's zero row must not win
    lld[3, 1, 0, 0] = -4.0                     # neither DBL (needs > -3) nor SNG (-5 > -6 + 2 fails): AMB
    c = A.make_calls(rows, cand, ll1, ll2, lld, al, grid)
    assert c.call[[0, 1, 3]].tolist() == [A.CALL_SNG, A.CALL_DBL, A.CALL_AMB]
    assert c.rho_sng1[0] == 0.1 and c.llk_sng1[0] == -8.0 and c.rho_sng2[0] == 0.2
    assert (c.dbl1[0], c.dbl2[0], c.alpha[0], c.rho_dbl[0], c.llk_dbl[0]) == (0, 2, 0.25, 0.1, -7.0)
    assert (c.dbl1[1], c.dbl2[1], c.alpha[1], c.rho_dbl[1], c.llr[1]) == (0, 2, 0.5, 0.0, 10.0)
    assert (c.dbl1[3], c.dbl2[3]) == (2, 1)
    assert [A.call_string(k, rows, c, samples) for k in (0, 1, 3)] == ["SNG-a", "DBL-a-c-0.500", "AMB-c-b-1-c/b-1"]
    p = tmp_path / "o.ambient_calls.tsv"
    A.write_calls_tsv(str(p), barcodes, samples, rows, c, np.array([7, 8, 0, 9]), np.array([10, 11, 0, 12]))
    lines = p.read_text().splitlines()
    assert lines[0] == A.CALLS_HEADER.rstrip("\n") and len(lines[0].split("\t")) == 17
    assert [l.split("\t")[0] for l in lines[1:]] == ["A-1", "G-1", "T-1"]          # byte-wise order, the barcode without a row left out
    assert lines[1].split("\t") == ["A-1", "DBL-a-c-0.500", "DBL-a-c-0.500", "a", "0.0000", "-30.00000", "c", "0.0000", "-30.50000", "a", "c", "0.500",
                                    "0.0000", "-20.00000", "10.00000", "8", "11"]
    assert lines[3].split("\t")[1:3] == ["SNG-a", "SNG-a"]
    # a barcode without any candidate pair: LLK.DBL = -inf, never DBL
    rows2 = A.BestRows(["SNG-a"], np.array([0], dtype=np.int32), np.array([0], dtype=np.int32), np.array([1], dtype=np.int32), np.array([1], dtype=np.int32))
    c2 = A.make_calls(rows2, A.candidates_from_best(rows2), ll1[:1], ll2[:1], np.zeros((1, 2, 2, 3)), al, grid)
    assert c2.dbl1[0] == -1 and c2.llk_dbl[0] == -np.inf and c2.call[0] != A.CALL_DBL


def test_dbl_alpha_checks_and_cli_errors(mods, capsys):
    A = mods["ambient"]
    assert A.dbl_alphas_from_run([0.0, 0.5]).tolist() == [0.5]
    assert A.dbl_alphas_from_run([0.5, 0.0, 0.1, 0.1]).tolist() == [0.1, 0.5]
    for bad in ([], [0.0, 0.5], [0.5, 0.4], [0.3, 0.3], [1.1], list(np.linspace(0.1, 0.9, 9))):
        with pytest.raises(ValueError):
            A.check_dbl_alphas(bad)
    with pytest.raises(ValueError):
        A.dbl_alphas_from_run([0.0])
    a = A.parse_args(["--pileup", "x", "--out", "y", "--doublets", "--alpha", "0", "0.1", "0.5"])
    assert a.doublets and a.dbl_alpha.tolist() == [0.1, 0.5]
    a = A.parse_args(["--pileup", "x", "--out", "y", "--doublets", "--dbl-alpha", "0.2", "0.4"])
    assert a.dbl_alpha.tolist() == [0.2, 0.4]
    assert not A.parse_args(["--pileup", "x", "--out", "y"]).doublets
    for argv in (["--dbl-alpha", "0.5"], ["--doublets", "--dbl-alpha", "0.0", "0.5"], ["--doublets", "--dbl-alpha", "0.5", "0.2"],
                 ["--doublets", "--alpha", "0"]):
        with pytest.raises(SystemExit):
            A.parse_args(["--pileup", "x", "--out", "y"] + argv)
    capsys.readouterr()


def test_mixed_generator_truth_and_counts(mods):
    synth = mods["synth"]
    rng = np.random.default_rng(8)
    S, V, B = 4000, 4, 40
    raw = synth.make_raw_genotypes(rng, S, V)
    dbl = np.arange(B) % 2 == 1
    rho = np.where(np.arange(B) % 4 < 2, 0.0, 0.4)
    sp, rho_o, al, a = synth.make_ambient_mixed_pileup(rng, raw.alleles, B, 0.5, 1.25, rho, dbl, 0.5)
    assert np.array_equal(rho_o, rho) and np.array_equal(al, np.where(dbl, 0.5, 0.0)) and a.shape == (S,)
    assert np.array_equal(sp.truth[:, 0], np.arange(B) % V)
    assert np.array_equal(sp.truth[:, 1] >= 0, dbl) and (sp.truth[dbl, 1] != sp.truth[dbl, 0]).all()
    assert sp.cell_pair_off[-1] == len(sp.pair_snp) == len(sp.pair_nrd) and sp.cell_read_off[-1] == len(sp.reads) == int(np.asarray(sp.pair_nrd).sum())
    assert np.array_equal(np.diff(sp.cell_read_off), np.add.reduceat(np.asarray(sp.pair_nrd, dtype=np.int64), sp.cell_pair_off[:-1]))
    assert abs(np.diff(sp.cell_pair_off).mean() / S - 0.5) < 0.02
    # the ALT fraction at SNPs where the first sample is hom-REF: ~0 for clean singlets, ~rho a for soupy ones, ~dosage of the second / 4 for doublets
    dosage = np.clip(raw.alleles, 0, 1).sum(axis=2)
    cell, snp, nrd, start = R.host_pairs(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd)
    first_alt = (np.asarray(sp.reads)[np.minimum(start, len(sp.reads) - 1)] >> 7) & (nrd > 0)
    homref = (dosage[snp, sp.truth[cell, 0]] == 0) & (nrd > 0)
    frac = lambda sel: first_alt[homref & sel[cell]].mean()
    clean, soupy, dclean = ~dbl & (rho == 0), ~dbl & (rho > 0), dbl & (rho == 0)
    exp_soup = 0.4 * a[snp[homref & soupy[cell]]].mean()
    assert frac(clean) < 0.01 and abs(frac(soupy) - exp_soup) < 0.03 and 0.1 < frac(dclean) < 0.4
    # the plain generator is untouched by the new one: same draws as before for the same seed
    r1, r2 = np.random.default_rng(9), np.random.default_rng(9)
    p1, _, _ = synth.make_ambient_pileup(r1, raw.alleles, 10, 0.1, 1.25, 0.2)
    p2, _, _ = synth.make_ambient_pileup(r2, raw.alleles, 10, 0.1, 1.25, 0.2)
    assert np.array_equal(p1.reads, p2.reads)
