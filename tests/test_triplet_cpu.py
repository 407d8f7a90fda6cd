"""CPU: the host side of the triplet calls (demuxlet_amd/triplet.py: share rules, decision rule, make_calls, writer, command-line argument
errors; synth.make_multiplet_pileup) and the numpy restatement (tests/triplet_ref.py) against an mpmath per-read product, against the
doublet and singlet restatements at zero shares, under permutation of the three donors, and as a caller of singlets, doublets and
triplets on its own.  No GPU compute is called."""
import numpy as np
import pytest

import ambient_dbl_ref as D
import ambient_ref as R
import triplet_ref as T3


@pytest.fixture(scope="module")
def mods():
    from demuxlet_amd import ambient, build, capi, engine, synth, triplet
    build.build()
    capi.load()
    return dict(ambient=ambient, capi=capi, engine=engine, synth=synth, triplet=triplet)


def one_cell(pairs, S):
    """A one-barcode CSR pileup from [(snp, read bytes)]."""
    po = np.array([0, len(pairs)], dtype=np.int64)
    return po, np.array([s for s, _ in pairs], dtype=np.int32), np.array([len(r) for _, r in pairs], dtype=np.int64), \
        np.concatenate([np.asarray(r, dtype=np.uint8) for _, r in pairs] + [np.zeros(0, dtype=np.uint8)])


def mp_profile(pairs, g, v1, v2, c, w, mat, err):
    """200-bit: sum over pairs of log(sum_lmn gp1_l gp2_m gpc_n prod over reads (pR (1 - p) + pA p))."""
    import mpmath as mp
    mp.mp.prec = 200
    tot = mp.mpf(0)
    for snp, rd in pairs:
        g1, g2, gc = g[snp, v1], g[snp, v2], g[snp, c]
        if len(rd) == 0 or not g1.any() or not g2.any() or not gc.any():
            continue
        L = mp.mpf(0)
        for l in range(3):
            for m in range(3):
                for n in range(3):
                    p = mp.mpf(0.5) * (mp.mpf(float(w[0])) * l + mp.mpf(float(w[1])) * m + mp.mpf(float(w[2])) * n)
                    f = mp.mpf(1)
                    for b in rd:
                        bq, alt = int(b) & 127, int(b) >> 7
                        pR = mp.mpf(float(err[bq])) / 3 if alt else mp.mpf(float(mat[bq]))
                        pA = mp.mpf(float(mat[bq])) if alt else mp.mpf(float(err[bq])) / 3
                        f *= pR * (1 - p) + pA * p
                    L += mp.mpf(float(g1[l])) * mp.mpf(float(g2[m])) * mp.mpf(float(gc[n])) * f
        tot += mp.log(L)
    return float(tot)


def test_restatement_against_mpmath(mods):
    """Small soft rows and a 400-read ALT-heavy pair on hom-REF hard rows, whose float64 product underflows."""
    mat, err = mods["engine"].phred_tables()
    rng = np.random.default_rng(3)
    S, V = 12, 4
    g = rng.dirichlet([1, 1, 1], size=(S, V)).astype(np.float32)
    g[5, :] = np.array([1.0, 0.0, 0.0], dtype=np.float32)
    g[5, 3] = np.array([0.0, 0.5, 0.5], dtype=np.float32)       # one sample that does explain the ALT reads
    g[7, 1] = 0.0                                   # all-zero row: skipped for slots that use sample 1, and for the third donor 1
    deep = np.where(rng.random(400) < 0.9, (1 << 7) | 40, 35).astype(np.uint8)
    pairs = [(1, [30, (1 << 7) | 20]), (3, [(1 << 7) | 0]), (5, deep), (7, [40, 40, (1 << 7) | 127]), (9, []), (10, [1, (1 << 7) | 127, 127])]
    assert np.prod([float(err[40]) / 3] * 360) == 0.0
    po, snp, nrd, reads = one_cell(pairs, S)
    shares = np.array([[1 / 3, 1 / 3, 1 / 3], [0.5, 0.25, 0.25], [0.7, 0.3, 0.0], [1.0, 0.0, 0.0]])
    base = np.array([[[0, 1], [2, 0], [-1, -1], [3, 2]]], dtype=np.int32)
    LL, ns, nr = T3.ref_triplet_profile(po, snp, nrd, reads, base, g, shares, mat, err)
    assert LL.shape == (1, 4, 4, V) and ns.shape == (1, 4, V)
    all_reads = 2 + 1 + 400 + 3 + 3
    assert ns[0, 0].tolist() == [4, 4, 4, 4] and ns[0, 1].tolist() == [5, 4, 5, 5] and not ns[0, 2].any()
    assert nr[0, 1].tolist() == [all_reads, all_reads - 3, all_reads, all_reads] and nr[0, 0, 0] == all_reads - 3
    assert not LL[0, 2].any() and np.isfinite(LL).all()
    assert LL[0, 0, 3, 0] < -2000 and LL[0, 0, 0, 3] > LL[0, 0, 0, 2] + 500      # the deep pair: hom-REF only, and with the ALT sample third
    for s in (0, 1, 3):
        for ti, w in enumerate(shares):
            for c in range(V):
                x = mp_profile(pairs, g, int(base[0, s, 0]), int(base[0, s, 1]), c, w, mat, err)
                assert abs(LL[0, s, ti, c] - x) <= 1e-10 * max(1.0, abs(x) * 1e-2), (s, w, c, LL[0, s, ti, c], x)


def small_pool(mods, seed, S, V, B, onehot_cols=()):
    synth, eng = mods["synth"], mods["engine"]
    rng = np.random.default_rng(seed)
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    for c in onehot_cols:
        g[:, c] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, size=S)]
    sp, _, _ = synth.make_multiplet_pileup(rng, raw.alleles, B, 0.2, 1.5, 1 + np.arange(B) % 3, (0.5, 0.3, 0.2))
    return rng, g, sp


def test_zero_third_share_is_the_doublet_restatement(mods):
    """w3 = 0 and exactly one-hot rows for c: the triplet restatement equals ambient_dbl_ref.ref_dbl_profile at rho = 0, alpha = w2."""
    mat, err = mods["engine"].phred_tables()
    S, V, B = 300, 5, 30
    rng, g, sp = small_pool(mods, 5, S, V, B, onehot_cols=(4,))
    v1 = (np.arange(B) % 3).astype(np.int32)
    base = np.stack([v1, (v1 + 1) % 4], axis=1).astype(np.int32)[:, None, :]
    csr = (sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads)
    LL, ns, nr = T3.ref_triplet_profile(*csr, base, g, [[0.7, 0.3, 0.0], [0.5, 0.5, 0.0]], mat, err)
    LD, nd, rd = D.ref_dbl_profile(*csr, base, g, np.zeros(S), [0.3, 0.5], [0.0], mat, err)
    assert np.array_equal(ns[:, 0, 4], nd[:, 0]) and np.array_equal(nr[:, 0, 4], rd[:, 0])
    assert np.abs(LL[:, 0, :, 4] - LD[:, 0, :, 0]).max() <= 1e-10


def test_single_share_is_the_singlet_restatement(mods):
    """w = (1, 0, 0) and one-hot rows for v2 and c: the singlet restatement of v1."""
    mat, err = mods["engine"].phred_tables()
    S, V, B = 300, 5, 30
    rng, g, sp = small_pool(mods, 7, S, V, B, onehot_cols=(3, 4))
    v1 = (np.arange(B) % 3).astype(np.int32)
    base = np.stack([v1, np.full(B, 3, dtype=np.int32)], axis=1)[:, None, :]
    csr = (sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads)
    LL, ns, nr = T3.ref_triplet_profile(*csr, base, g, [[1.0, 0.0, 0.0]], mat, err)
    L1, n1, r1 = R.ref_profile(*csr, v1, g, np.zeros(S), [0.0], mat, err)
    assert np.array_equal(ns[:, 0, 4], n1) and np.array_equal(nr[:, 0, 4], r1)
    assert np.abs(LL[:, 0, 0, 4] - L1[:, 0]).max() <= 1e-10


def test_permutation_symmetry_of_the_restatement(mods):
    """((a, b), c, (w1, w2, w3)) = ((a, c), b, (w1, w3, w2)) = ((b, a), c, (w2, w1, w3))."""
    mat, err = mods["engine"].phred_tables()
    S, V, B = 200, 5, 12
    rng, g, sp = small_pool(mods, 6, S, V, B)
    csr = (sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads)
    a, b, c = 0, 2, 3
    tile = lambda p: np.tile(np.array([[p]], dtype=np.int32), (B, 1, 1))
    w = [0.5, 0.3, 0.2]
    x, _, _ = T3.ref_triplet_profile(*csr, tile((a, b)), g, [w], mat, err)
    y, _, _ = T3.ref_triplet_profile(*csr, tile((a, c)), g, [[w[0], w[2], w[1]]], mat, err)
    z, _, _ = T3.ref_triplet_profile(*csr, tile((b, a)), g, [[w[1], w[0], w[2]]], mat, err)
    assert x[:, 0, 0, c].any()
    assert np.abs(x[:, 0, 0, c] - y[:, 0, 0, b]).max() <= 1e-9 and np.abs(x[:, 0, 0, c] - z[:, 0, 0, c]).max() <= 1e-9


def test_share_rules(mods):
    T = mods["triplet"]
    d = T.default_shares()
    assert d.shape == (4, 3) and d[0].tolist() == [1 / 3, 1 / 3, 1 / 3] and d[1:].tolist() == [[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]]
    assert np.array_equal(T.check_shares(d), d)
    assert T.check_shares([[0.7, 0.3, 0.0]], allow_zero=True).tolist() == [[0.7, 0.3, 0.0]]
    for bad in ([], [[0.5, 0.5]], [[0.7, 0.3, 0.0]], [[0.5, 0.25, 0.25], [0.5, 0.25, 0.25]], [[0.5, 0.3, 0.3]], [[1.2, -0.1, -0.1]],
                [[0.5, 0.25, 0.25 + 1e-9]], [[0.2, 0.3, 0.5]] * 9, [[np.nan, 0.5, 0.5]]):
        with pytest.raises(ValueError):
            T.check_shares(bad)
    nine = [[0.1 + 0.01 * k, 0.5, 0.4 - 0.01 * k] for k in range(9)]
    with pytest.raises(ValueError):
        T.check_shares(nine)
    assert len(T.check_shares(nine[:8])) == 8
    assert T.shares_string(d[0]) == "0.333/0.333/0.333"


def test_decision_rule_at_its_thresholds(mods):
    T, A = mods["triplet"], mods["ambient"]
    s1 = np.array([-100.0] * 7)
    s2 = np.array([-103.0] * 7)
    d = np.array([-90.0, -90.0, -90.0, -120.0, -120.0, -np.inf, -90.0])
    t = np.array([-88.0, -88.0 + 1e-9, -89.0, -98.0, -98.0 + 1e-9, -97.0, -np.inf])
    got = T.decide(s1, s2, d, t).tolist()
    # TRP needs LLK.TRP > max(LLK.DBL, LLK.SNG1) + 2: exactly +2 is not a triplet, and ambient.decide then applies unchanged
    assert got == [A.CALL_DBL, T.CALL_TRP, A.CALL_DBL, A.CALL_SNG, T.CALL_TRP, T.CALL_TRP, A.CALL_DBL]
    assert T.CALL_TRP not in (A.CALL_SNG, A.CALL_DBL, A.CALL_AMB) and A.CALL_MARGIN == 2.0


def test_make_calls_and_writer(mods, tmp_path):
    T, A = mods["triplet"], mods["ambient"]
    samples = ["a", "b-1", "c", "d"]
    barcodes = ["T-1", "A-1", "C-1", "G-1", "B-1"]
    i32 = lambda x: np.array(x, dtype=np.int32)
    rows = A.BestRows(["SNG-a", "DBL-a-c-0.500", "", "SNG-c", "SNG-a"], i32([0, 0, -1, 2, 0]), i32([1, 2, -1, 1, 0]), i32([0, 0, -1, 2, 1]), i32([2, 2, -1, 0, 1]))
    cand = A.candidates_from_best(rows)
    assert cand.tolist() == [[[0, 2], [0, 1]], [[0, 2], [-1, -1]], [[-1, -1], [-1, -1]], [[2, 0], [2, 1]], [[-1, -1], [-1, -1]]]
    sh = T.default_shares()
    al = np.array([0.25, 0.5])
    l1 = np.array([-10.0, -30.0, 0.0, -5.0, -3.0])
    l2 = np.array([-20.0, -30.5, 0.0, -6.0, -3.0])
    lld = np.full((5, 2, 2), -50.0)
    lld[1, 0, 1] = -20.0
    lld[1, 1] = 0.0                            # an unused slot's zero row must not win
    llt = np.full((5, 2, 4, 4), -60.0)
    llt[0, 0, :, 0] = 0.0                      # c = v1 and c = v2 are ignored
    llt[0, 0, :, 2] = 0.0
    llt[0, 1, 2, 3] = -7.0                     # a tie: the lowest (slot, share, c) index is reported
    llt[0, 0, 1, 3] = -7.0
    llt[0, 1, 1, 2] = -7.0
    llt[1, 0, 3, 1] = -18.0                    # exactly LLK.DBL + 2: not a triplet
    llt[1, 1] = 0.0                            # unused slot
    llt[3, 1, 0, 3] = -2.0                     # slot 1 = (c, b-1) with d
    llt[4] = 0.0                               # no slot at all
    c = T.make_calls(rows, cand, l1, l2, lld, al, llt)
    assert c.call[[0, 1, 3, 4]].tolist() == [T.CALL_TRP, A.CALL_DBL, T.CALL_TRP, A.CALL_AMB]
    assert (c.trp1[0], c.trp2[0], c.trp3[0], c.share[0], c.llk_trp[0], c.llr[0]) == (0, 2, 3, 1, -7.0, 3.0)
    assert (c.trp1[1], c.trp2[1], c.trp3[1], c.share[1], c.llk_trp[1], c.llr[1]) == (0, 2, 1, 3, -18.0, 2.0)
    assert (c.dbl1[1], c.dbl2[1], c.alpha[1], c.llk_dbl[1]) == (0, 2, 0.5, -20.0)
    assert (c.trp1[3], c.trp2[3], c.trp3[3], c.share[3]) == (2, 1, 3, 0)
    assert c.trp1[4] == -1 and c.trp3[4] == -1 and c.llk_trp[4] == -np.inf and c.dbl1[4] == -1 and c.llk_dbl[4] == -np.inf
    assert [T.call_string(k, rows, c, samples, sh) for k in (0, 1, 3)] == ["TRP-a-c-d-0.500/0.250/0.250", "DBL-a-c-0.500", "TRP-c-b-1-d-0.333/0.333/0.333"]
    p = tmp_path / "o.triplet.tsv"
    T.write_triplet_tsv(str(p), barcodes, samples, rows, c, sh, np.array([7, 8, 0, 9, 4]), np.array([10, 11, 0, 12, 5]))
    lines = p.read_text().splitlines()
    assert lines[0] == T.TRIPLET_HEADER.rstrip("\n")
    assert lines[0].split("\t") == ["BARCODE", "BEST", "CALL", "SNG.1ST", "LLK.SNG1", "SNG.2ND", "LLK.SNG2", "DBL.1ST", "DBL.2ND", "ALPHA", "LLK.DBL", "TRP.1ST",
                                    "TRP.2ND", "TRP.3RD", "SHARES", "LLK.TRP", "LLR", "N.SNP", "N.READ"]
    assert [l.split("\t")[0] for l in lines[1:]] == ["A-1", "B-1", "G-1", "T-1"]          # byte-wise order, the barcode without a row left out
    assert lines[1].split("\t") == ["A-1", "DBL-a-c-0.500", "DBL-a-c-0.500", "a", "-30.00000", "c", "-30.50000", "a", "c", "0.500", "-20.00000", "a", "c", "b-1",
                                    "0.250/0.250/0.500", "-18.00000", "2.00000", "8", "11"]
    assert lines[2].split("\t")[7:17] == [".", ".", ".", ".", ".", ".", ".", ".", ".", "."]
    assert lines[4].split("\t")[1:3] == ["SNG-a", "TRP-a-c-d-0.500/0.250/0.250"]
    # two samples: no third donor exists, whatever the profile holds
    rows2 = A.BestRows(["SNG-a"], i32([0]), i32([1]), i32([0]), i32([1]))
    c2 = T.make_calls(rows2, A.candidates_from_best(rows2), l1[:1], l2[:1], np.full((1, 2, 2), -50.0), al, np.zeros((1, 2, 4, 2)))
    assert c2.trp1[0] == -1 and c2.llk_trp[0] == -np.inf and c2.call[0] == A.CALL_SNG


def test_cli_argument_errors(mods, capsys):
    T = mods["triplet"]
    a = T.parse_args(["--pileup", "x", "--out", "y"])
    assert np.array_equal(a.shares, T.default_shares()) and a.dbl_alpha.tolist() == [0.5] and a.best is None and not a.fast
    a = T.parse_args(["--pileup", "x", "--out", "y", "--shares", "0.6,0.2,0.2", "0.2,0.6,0.2", "--alpha", "0", "0.3", "0.5", "--best", "z.best"])
    assert a.shares.tolist() == [[0.6, 0.2, 0.2], [0.2, 0.6, 0.2]] and a.dbl_alpha.tolist() == [0.3, 0.5] and a.best == "z.best"
    assert T.parse_args(["--pileup", "x", "--out", "y", "--dbl-alpha", "0.2", "0.4"]).dbl_alpha.tolist() == [0.2, 0.4]
    for argv in (["--shares", "0.5,0.5"], ["--shares", "0.5,0.5,0.0"], ["--shares", "0.5,0.3,0.3"], ["--shares", "a,b,c"],
                 ["--shares", "0.5,0.25,0.25", "0.5,0.25,0.25"], ["--shares"] + ["0.5,0.25,0.25"] * 9, ["--alpha", "0"],
                 ["--dbl-alpha", "0.0", "0.5"], ["--dbl-alpha", "0.5", "0.2"], ["--bogus"]):
        with pytest.raises(SystemExit):
            T.parse_args(["--pileup", "x", "--out", "y"] + argv)
    with pytest.raises(SystemExit):
        T.parse_args(["--out", "y"])
    capsys.readouterr()


def test_multiplet_generator(mods):
    synth = mods["synth"]
    rng = np.random.default_rng(8)
    S, V, B = 4000, 5, 60
    raw = synth.make_raw_genotypes(rng, S, V)
    kinds = 1 + np.arange(B) % 3
    shares = np.where((np.arange(B) % 2 == 0)[:, None], np.array([[0.5, 0.25, 0.25]]), np.array([[0.6, 0.3, 0.1]]))
    sp, t3, w = synth.make_multiplet_pileup(rng, raw.alleles, B, 0.5, 1.25, kinds, shares)
    assert t3.shape == (B, 3) and w.shape == (B, 3) and t3.dtype == np.int32
    assert np.array_equal(t3[:, 0], np.arange(B) % V) and np.array_equal((t3 >= 0).sum(axis=1), kinds) and np.array_equal(sp.truth, t3[:, :2])
    for c in range(B):
        d = t3[c, :kinds[c]]
        assert len(set(d.tolist())) == kinds[c] and (t3[c, kinds[c]:] == -1).all() and (w[c, kinds[c]:] == 0).all()
    assert np.allclose(w.sum(axis=1), 1.0) and w[0].tolist() == [1.0, 0.0, 0.0] and np.allclose(w[1], [2 / 3, 1 / 3, 0.0]) and w[2].tolist() == [0.5, 0.25, 0.25]
    assert {int(x) for x in t3[kinds == 3, 2]} == set(range(V))                  # every sample turns up as a third donor
    assert sp.pair_snp is not None
    assert sp.cell_pair_off[-1] == len(sp.pair_snp) == len(sp.pair_nrd) and sp.cell_read_off[-1] == len(sp.reads) == int(np.asarray(sp.pair_nrd).sum())
    assert np.array_equal(np.diff(sp.cell_read_off), np.add.reduceat(np.asarray(sp.pair_nrd, dtype=np.int64), sp.cell_pair_off[:-1]))
    assert abs(np.diff(sp.cell_pair_off).mean() / S - 0.5) < 0.02
    # the ALT fraction of first reads by genotype configuration: sum_k w_k dosage_k / 2, for every configuration of the 0.6 / 0.3 / 0.1 triplets
    # and 2 : 1 doublets (a base error moves a read by ~1e-2 at most: bq >= 13 errs 5 % of the time and a third of those flip the allele)
    dosage = np.clip(raw.alleles, 0, 1).sum(axis=2)
    cell, snp, nrd, start = R.host_pairs(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd)
    first_alt = ((np.asarray(sp.reads)[np.minimum(start, len(sp.reads) - 1)] >> 7) != 0) & (nrd > 0)
    d3 = np.stack([dosage[snp, np.maximum(t3[cell, k], 0)] for k in range(3)], axis=1)
    expect = (w[cell] * d3).sum(axis=1) / 2.0
    assert first_alt[(nrd > 0) & (kinds[cell] == 1) & (d3[:, 0] == 0)].mean() < 0.02
    seen = 0
    for kind in (2, 3):
        sel = (nrd > 0) & (kinds[cell] == kind) & (cell % 2 == 1)
        for cfg in np.unique(d3[sel][:, :kind], axis=0):
            grp = sel & (d3[:, :kind] == cfg).all(axis=1)
            n, pe = int(grp.sum()), float(expect[grp][0])
            if n < 200:
                continue
            seen += 1
            assert abs(first_alt[grp].mean() - pe) < 4.0 * np.sqrt(max(pe * (1 - pe), 0.01) / n) + 0.02, (kind, cfg, n, pe, first_alt[grp].mean())
    assert seen >= 30                                                            # 9 doublet and 27 triplet configurations, the rare ones left out
    # the dense layout, and bad arguments
    dp, _, _ = synth.make_multiplet_pileup(rng, raw.alleles[:50], 7, 1.0, 1.5, 3, (1 / 3, 1 / 3, 1 / 3), dense_layout=True, quals="edges")
    assert dp.pair_snp is None and dp.cell_pair_off.tolist() == [50 * k for k in range(8)]
    sq, _, _ = synth.make_multiplet_pileup(rng, raw.alleles[:50], 7, 1.0, 1.5, 3, (1 / 3, 1 / 3, 1 / 3))
    assert sq.pair_snp is not None
    for kw in (dict(kinds=4), dict(kinds=0), dict(shares=(0.0, 0.5, 0.5), kinds=1), dict(shares=(-0.5, 1.0, 0.5))):
        with pytest.raises(ValueError):
            synth.make_multiplet_pileup(rng, raw.alleles[:50], 4, 1.0, 1.5, **{"kinds": 3, "shares": (0.5, 0.25, 0.25), **kw})
    with pytest.raises(ValueError):
        synth.make_multiplet_pileup(rng, raw.alleles[:50, :2], 4, 1.0, 1.5, 3, (0.5, 0.25, 0.25))
    # the older generators are untouched: same draws as before for the same seed
    r1, r2 = np.random.default_rng(9), np.random.default_rng(9)
    p1, _, _ = synth.make_ambient_pileup(r1, raw.alleles, 10, 0.1, 1.25, 0.2)
    p2, _, _ = synth.make_ambient_pileup(r2, raw.alleles, 10, 0.1, 1.25, 0.2)
    assert np.array_equal(p1.reads, p2.reads)


def recovery_pool(synth, eng, rng, S, V, n_sng, n_dbl, n_trp, delta, rbar):
    """Singlets, doublets (half 0.5 / 0.5, half 0.7 / 0.3) and triplets (half even thirds, half 0.5 / 0.25 / 0.25), interleaved."""
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    kinds = np.concatenate([np.full(n_sng, 1), np.full(n_dbl, 2), np.full(n_trp, 3)])
    half = lambda n: np.arange(n) % 2 == 1
    shares = np.concatenate([np.tile([[1.0, 0.0, 0.0]], (n_sng, 1)),
                             np.where(half(n_dbl)[:, None], [[0.7, 0.3, 0.0]], [[0.5, 0.5, 0.0]]),
                             np.where(half(n_trp)[:, None], [[0.5, 0.25, 0.25]], [[1 / 3, 1 / 3, 1 / 3]])])
    order = rng.permutation(len(kinds))
    sp, t3, w = synth.make_multiplet_pileup(rng, raw.alleles, len(kinds), delta, rbar, kinds[order], shares[order])
    return g, sp, t3, kinds[order]


def test_recovery_with_the_restatement_alone(mods):
    """6 donors, ~1 000 covered SNPs per barcode: 20 singlets, 30 doublets (half 0.7 / 0.3), 20 triplets (half 0.5 / 0.25 / 0.25).  The base
    pair is the restatement's best doublet over all 15 pairs at alpha 0.25 / 0.5 / 0.75; no singlet or doublet is called TRP and at least
    19 of 20 triplets are called TRP with their three donors.

    Seed 41: 20 of 20 triplets right; the smallest |LLR - 2| over the 70 barcodes is 18.0."""
    T, A, synth, eng = mods["triplet"], mods["ambient"], mods["synth"], mods["engine"]
    mat, err = eng.phred_tables()
    rng = np.random.default_rng(41)
    S, V = 2000, 6
    g, sp, t3, kinds = recovery_pool(synth, eng, rng, S, V, 20, 30, 20, 0.5, 1.2)
    B = len(kinds)
    assert 900 < np.median(np.diff(sp.cell_pair_off)) < 1100
    csr = (sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads)
    zeros, rho0 = np.zeros(S), [0.0]
    sng = np.stack([R.ref_profile(*csr, np.full(B, v, dtype=np.int32), g, zeros, rho0, mat, err)[0][:, 0] for v in range(V)], axis=1)      # [B][V]
    top = np.argsort(-sng, axis=1, kind="stable")
    pairs = np.array([(a, b) for a in range(V) for b in range(a + 1, V)], dtype=np.int32)
    dal = np.array([0.25, 0.5, 0.75])
    LD, _, _ = D.ref_dbl_profile(*csr, np.tile(pairs[None], (B, 1, 1)), g, zeros, dal, rho0, mat, err)                                   # [B][15][3][1]
    bp = pairs[np.argmax(LD[:, :, :, 0].max(axis=2), axis=1)]
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
    rows = A.BestRows(["?"] * B, i32(top[:, 0]), i32(top[:, 1]), i32(bp[:, 0]), i32(bp[:, 1]))
    cand = A.candidates_from_best(rows)
    ll1 = sng[np.arange(B), top[:, 0]]
    ll2 = sng[np.arange(B), top[:, 1]]
    lld, _, _ = D.ref_dbl_profile(*csr, cand, g, zeros, dal, rho0, mat, err)
    llt, _, _ = T3.ref_triplet_profile(*csr, cand, g, T.default_shares(), mat, err)
    c = T.make_calls(rows, cand, ll1, ll2, lld[:, :, :, 0], dal, llt)
    is_trp = c.call == T.CALL_TRP
    named = np.array([{int(c.trp1[k]), int(c.trp2[k]), int(c.trp3[k])} == set(t3[k].tolist()) for k in range(B)])
    margin = np.abs(c.llr - A.CALL_MARGIN).min()
    print(f"TRP among singlets {int(is_trp[kinds == 1].sum())}, doublets {int(is_trp[kinds == 2].sum())}; triplets right "
          f"{int((is_trp & named)[kinds == 3].sum())} of {int((kinds == 3).sum())}; smallest |LLR - 2| = {margin:.1f}")
    assert not is_trp[kinds < 3].any()
    assert (is_trp & named)[kinds == 3].sum() >= 19
