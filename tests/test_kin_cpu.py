"""CPU: the joint-genotype-table contract (include/dmx.h, "Joint genotype tables") through its host emulator tests/kin_emul.cpp, and the
pure functions of demuxlet_amd/kin.py: statistics, flags, the expected log-likelihood ratio, the assignment solver, the readers, the
alignment and the command line's errors.  No GPU."""
import numpy as np
import pytest

import kin_ref as KR


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return KR.build(tmp_path_factory.mktemp("kin_emul"))


@pytest.fixture(scope="module")
def kin():
    from demuxlet_amd import kin
    return kin


@pytest.fixture(scope="module")
def tables():
    from demuxlet_amd import build, engine
    build.build()
    return engine.phred_tables()


@pytest.fixture(scope="module")
def soft(emu):
    """A soft edge matrix pair, its images and its three tables (contract, descending, multiply + add)."""
    rng = np.random.default_rng(5)
    S, VA, VB = 3000, 5, 4
    ga, gb, c = KR.edge_matrix(rng, S, VA), KR.edge_matrix(rng, S, VB), KR.edge_weight(rng, S)
    wa, _ = emu.rows(ga, c)
    rb, _ = emu.rows(gb)
    out = dict(S=S, wa=wa, rb=rb)
    for name, v in (("T", 0), ("desc", KR.DESCENDING), ("muladd", KR.MUL_ADD)):
        emu.variant(v)
        out[name] = emu.table(wa, rb)
    emu.variant(0)
    out["ld"] = KR.table_longdouble(wa, rb)
    return out


def test_accuracy_against_longdouble(soft):
    """Every entry within S u / (1 - S u) T of the long-double restatement on the emulator's own rounded operands."""
    err = np.abs(soft["T"].astype(np.longdouble) - soft["ld"])
    assert (soft["ld"] > 0).any()
    assert (err <= KR.chain_bound(soft["S"], soft["ld"])).all()


def test_wrong_variants_differ_in_bits_inside_the_bound(soft):
    """The bit test has teeth: descending order and a separate multiply and add each change at least one entry's bits, and both stay
    inside the accuracy bound (twice the roundings for multiply + add)."""
    for name, k in (("desc", 1), ("muladd", 2)):
        assert (KR.bits(soft[name]) != KR.bits(soft["T"])).any(), name
        err = np.abs(soft[name].astype(np.longdouble) - soft["ld"])
        assert (err <= KR.chain_bound(k * soft["S"], soft["ld"])).all(), name


def test_null_weight_is_ones_and_entries_do_not_depend_on_the_panel(emu):
    rng = np.random.default_rng(6)
    ga, gb = KR.edge_matrix(rng, 257, 4), KR.edge_matrix(rng, 257, 3)
    T0, na, nb = emu.compare(ga, gb)
    T1, _, _ = emu.compare(ga, gb, np.ones(257))
    assert (KR.bits(T0) == KR.bits(T1)).all()
    Tp, _, _ = emu.compare(ga[:, 2:3], gb[:, 1:2])
    assert (KR.bits(Tp[0, 0]) == KR.bits(T0[2, 1])).all()
    assert emu.compare(ga[:0], gb[:0])[0].shape == (4, 3, 4, 4) and not emu.compare(ga[:0], gb[:0])[0].any()


def test_row_transform(emu):
    """Each kind of edge row: validity, the zero vector of an invalid row, IEEE quotients of a valid one, the weight's single rounding."""
    g = np.array([KR.SPECIAL_ROWS], dtype=np.float32)                   # [1][14][3]
    img, valid = emu.rows(g)
    assert valid[0].tolist() == KR.SPECIAL_VALID
    for k, ok in enumerate(KR.SPECIAL_VALID):
        if not ok:
            assert (KR.bits(img[0, k]) == 0).all()                      # +0.0 four times
        else:
            w = g[0, k].astype(np.float64)
            s = (w[0] + w[1]) + w[2]
            assert (KR.bits(img[0, k]) == KR.bits(np.array([w[0] / s, w[1] / s, w[2] / s, 1.0]))).all()
    assert img[0, 13].tolist() == [0.2, 0.3, 0.5, 1.0]                  # (2, 3, 5) is normalised
    assert img[0, 9, :3].tolist() == [1 / 3, 1 / 3, 1 / 3]              # float32 subnormals widen exactly
    c = np.array([0.3])
    wimg, _ = emu.rows(g, c)
    assert (KR.bits(wimg) == KR.bits(0.3 * img)).all()
    assert wimg[0, 1, 3] == 0.3 and wimg[0, 0, 3] == 0.0


def test_statistics_on_hand_made_tables(kin):
    def table(J):
        t = np.zeros((4, 4)); t[:3, :3] = J
        t[:3, 3] = np.sum(J, axis=1); t[3, :3] = np.sum(J, axis=0); t[3, 3] = np.sum(J)
        return t

    ident = table(np.diag([50.0, 30.0, 20.0]))
    st = kin.pair_stats(ident)
    assert st["N"] == 100 and st["IBS0"] == 0 and st["IBS2"] == 1 and st["DISC"] == 0 and st["KIN"] == 0.5 and abs(st["R"] - 1) < 1e-12
    opp = table([[0, 0, 10.0], [0, 0, 0], [10.0, 0, 0]])
    st = kin.pair_stats(opp)
    assert st["IBS0"] == 1 and st["IBS2"] == 0 and abs(st["R"] + 1) < 1e-12 and np.isnan(st["KIN"])      # no heterozygote: 0 / 0
    J = np.array([[30.0, 12, 2], [10, 25, 6], [1, 5, 9]])
    st, ref = kin.pair_stats(table(J)), KR.ref_stats(table(J))
    for k in ref:
        assert abs(st[k] - ref[k]) < 1e-12, k
    assert ref["KIN"] == (25 - 2 * 3) / (41 + 42) and ref["IBS0"] == 3 / 100
    many = kin.pair_stats(np.stack([ident, table(J)]).reshape(2, 1, 4, 4))
    assert many["KIN"].shape == (2, 1) and many["KIN"][0, 0] == 0.5
    empty = kin.pair_stats(np.zeros((4, 4)))
    assert np.isnan(empty["KIN"]) and np.isnan(empty["IBS0"]) and empty["N"] == 0


def test_flags(kin):
    f = kin.flag_of
    assert f(500, 0.5, 40.0, 2.0, 100) == "DUP" and f(500, 0.5, 0.0, 2.0, 100) == "DUP,INSEP"
    assert f(500, 0.25, 40.0, 2.0, 100) == "REL1" and f(500, 0.12, 1.9, 2.0, 100) == "REL2,INSEP"
    assert f(500, 0.05, 40.0, 2.0, 100) == "." and f(500, 0.05, 1.0, 2.0, 100) == "INSEP" and f(500, 0.05, None, 2.0, 100) == "."
    assert f(99, 0.5, 0.0, 2.0, 100) == "LOWN" and f(float("nan"), 0.5, 0.0, 2.0, 100) == "LOWN"
    assert f(500, 0.354, 40.0, 2.0, 100) == "REL1" and f(500, 0.0884, 40.0, 2.0, 100) == "." and f(500, float("nan"), 40.0, 2.0, 100) == "."


def test_pedigree_bands(emu, kin):
    """S = 4000 hard rows, one fixed seed: the duplicate's KIN is 0.5 exactly, parent-child and full siblings lie in (0.177, 0.354),
    half-siblings in (0.0884, 0.177), everybody else below 0.0884; the flag of every pair is its band."""
    S = 4000
    g = KR.pedigree(np.random.default_rng(2024), S)
    T, nv, _ = emu.compare(g)
    assert (nv == S).all()
    st = kin.pair_stats(T)
    seen = set()
    for a, na in enumerate(KR.PEDIGREE):
        for b, nb in enumerate(KR.PEDIGREE):
            if a == b:
                continue
            band, k = KR.expected_band(na, nb), st["KIN"][a, b]
            seen.add(band)
            assert abs(k - KR.ref_stats(T[a, b])["KIN"]) < 1e-12
            if band == "DUP":
                assert k == 0.5 and st["DISC"][a, b] == 0.0
            elif band == "REL1":
                assert kin.KIN_REL1 < k < kin.KIN_DUP, (na, nb, k)
            elif band == "REL2":
                assert kin.KIN_REL2 < k < kin.KIN_REL1, (na, nb, k)
            else:
                assert k < kin.KIN_REL2, (na, nb, k)
            assert kin.flag_of(st["N"][a, b], k, None, 2.0, 100) == band
    assert seen == {"DUP", "REL1", "REL2", "."}
    ia, ib = KR.PEDIGREE.index("A"), KR.PEDIGREE.index("B")
    assert kin.flag_of(st["N"][ia, ib], st["KIN"][ia, ib], None, 2.0, 100) == "."


def test_expected_llr_against_simulated_cells(emu, kin, tables):
    """200 cells of donor A with reads drawn from the model at the pool's coverage: the mean realised llk_A - llk_k1 agrees with LLR.AB
    within 4 standard errors of that mean (taken from the sample), and KL is the restatement's."""
    mat, err = tables
    rng = np.random.default_rng(77)
    S = 1500
    g = KR.pedigree(rng, S)
    ia, ib = KR.PEDIGREE.index("A"), KR.PEDIGREE.index("k1")
    c = rng.uniform(0.02, 0.2, size=S)
    bqs = np.array([20, 30, 37])
    hist = np.zeros(128); hist[bqs] = 1.0
    kl = kin.kl_table(mat, err, hist)
    assert np.allclose(kl, KR.ref_kl(mat, err, hist), rtol=1e-12, atol=1e-15)
    assert (np.diag(kl) == 0).all() and (kl[~np.eye(3, dtype=bool)] > 0).all()
    Tc, _, _ = emu.compare(g[:, [ia, ib]], c=c)
    want = kin.llr(Tc, kl)[0, 1]
    xa, xb = g[:, ia].argmax(axis=1), g[:, ib].argmax(axis=1)
    assert abs(want - sum(c[i] * kl[xa[i], xb[i]] for i in range(S))) < 1e-9 * want
    d = KR.simulate_llr(rng, xa, xb, c, mat, err, bqs, 200)
    se = d.std(ddof=1) / np.sqrt(len(d))
    print(f"LLR.AB {want:.4f}, simulated mean {d.mean():.4f}, SE {se:.4f}")
    assert abs(d.mean() - want) <= 4 * se
    assert kin.llr(Tc, kl)[0, 0] == 0.0                                 # a donor against itself


def test_kl_is_finite_at_every_quality(kin, tables):
    """The singlet pass's floor keeps the logs finite even where a match probability is zero; an empty histogram gives zeros."""
    mat, err = tables
    kl = kin.kl_table(mat, err, np.ones(128))
    assert np.isfinite(kl).all() and (np.diag(kl) == 0).all() and (kl >= 0).all()
    assert np.allclose(kl, KR.ref_kl(mat, err, np.ones(128)), rtol=1e-12, atol=1e-15)
    assert not kin.kl_table(mat, err, np.zeros(128)).any()


def test_pool_weight(kin):
    from demuxlet_amd import engine
    # three barcodes over four SNPs: reads per SNP (3, 0, 1, 1); the third barcode has a pair without stored reads only
    pl = engine.HostPileup(3, 4, np.array([0, 2, 4, 5]), np.array([0, 3, 5, 5]), np.array([0, 2, 0, 3, 1], dtype=np.int32),
                           np.array([2, 1, 1, 1, 0], dtype=np.uint8), np.array([30, 30 | 128, 20, 30, 40 | 128], dtype=np.uint8),
                           np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32))
    c, hist, n_bc = kin.pool_weight(pl)
    assert n_bc == 2 and c.tolist() == [1.5, 0.0, 0.5, 0.5] and hist[30] == 3 and hist[20] == 1 and hist[40] == 1 and hist.sum() == 5


def test_assignment_against_brute_force(kin):
    """Every shape up to 6 x 6, rectangular both ways, with masked pairs and negative gains."""
    rng = np.random.default_rng(9)
    for nA in range(1, 7):
        for nB in range(1, 7):
            for rep in range(4):
                gain = rng.uniform(-0.2, 0.5, size=(nA, nB))
                allowed = None if rep == 0 else rng.random((nA, nB)) < (0.9, 0.6, 0.3)[rep - 1]
                out = kin.assign_max(gain, allowed)
                used = out[out >= 0]
                assert len(set(used.tolist())) == len(used)
                for i, j in enumerate(out):
                    assert j < 0 or (gain[i, j] > 0 and (allowed is None or allowed[i, j]))
                tot = sum(gain[i, j] for i, j in enumerate(out) if j >= 0)
                assert abs(tot - KR.brute_assign(gain, allowed)) < 1e-12, (nA, nB, rep)
    assert kin.assign_max(np.zeros((0, 3))).shape == (0,) and kin.assign_max(np.full((2, 2), -1.0)).tolist() == [-1, -1]
    g = np.array([[0.5, 0.45], [0.45, 0.1]])                              # the greedy choice (0, 0) loses
    assert kin.assign_max(g).tolist() == [1, 0]


def _write_refined(refine, path, keys, ids, gp, covered):
    S, V = gp.shape[:2]
    z = np.zeros((S, V, 3)); n = covered.astype(np.int64)
    refine.write_refined_tsv(str(path), keys, ids, z, n, n, n, gp)


def test_readers_and_alignment(kin, tmp_path):
    from demuxlet_amd import refine
    keys = [(1, 100, "A", "C"), (1, 200, "G", "T"), (2, 50, "C", "T"), (2, 60, "T", "A")]
    gp = np.random.default_rng(3).dirichlet(np.ones(3), size=(4, 2)).astype(np.float32)
    covered = np.array([[1, 1], [1, 0], [0, 0], [0, 1]], dtype=bool)
    _write_refined(refine, tmp_path / "a.refined.tsv", keys, ["CLUST0", "CLUST1"], gp, covered)
    k, ids, g = kin.load_matrix(str(tmp_path / "a.refined.tsv"))
    assert ids == ["CLUST0", "CLUST1"] and k == [("1", 100, "A", "C"), ("1", 200, "G", "T"), ("2", 60, "T", "A")]     # SNP (2, 50) has no row
    assert g.shape == (3, 2, 3) and not g[1, 1].any() and not g[2, 0].any()                     # unlisted rows are all zero
    assert np.allclose(g[0], gp[0], rtol=1e-5) and np.allclose(g[2, 1], gp[3, 1], rtol=1e-5)
    # B: the first SNP shared, the second with REF / ALT swapped, one SNP of its own
    kb = [("1", 100, "A", "C"), ("1", 200, "T", "G"), ("3", 7, "A", "G")]
    gb = np.ones((3, 1, 3), dtype=np.float32)
    keys2, ga2, gb2, info = kin.align(k, g, kb, gb)
    assert info == dict(shared=1, only_a=1, only_b=1, allele_mismatch=1)
    assert keys2 == [("1", 100, "A", "C"), ("2", 60, "T", "A"), ("3", 7, "A", "G")]
    assert ga2.shape == (3, 2, 3) and gb2.shape == (3, 1, 3)
    assert (ga2[0] == g[0]).all() and (ga2[1] == g[2]).all() and not ga2[2].any()
    assert gb2[0].all() and not gb2[1].any() and gb2[2].all()
    on, miss = kin.onto_keys(kin.snp_keys(keys), k + [("9", 1, "A", "C")], np.concatenate([g, g[:1]]))
    assert miss == 1 and on.shape == (4, 2, 3) and (on[0] == g[0]).all() and not on[2].any() and (on[3] == g[2]).all()
    (tmp_path / "bad.tsv").write_text("RID\tPOS\tREF\n")
    with pytest.raises(ValueError, match="no ALT column"):
        kin.read_genotype_tsv(str(tmp_path / "bad.tsv"))
    (tmp_path / "short.tsv").write_text(refine.REFINED_HEADER + "1\t5\tA\n")
    with pytest.raises(ValueError, match="fields"):
        kin.read_genotype_tsv(str(tmp_path / "short.tsv"))


def test_command_line_errors(kin, tmp_path, capsys):
    with pytest.raises(SystemExit):
        kin.main(["--out", str(tmp_path / "o")])                       # --pileup is required
    with pytest.raises(SystemExit):
        kin.main(["--pileup", "x", "--out", str(tmp_path / "o"), "--margin", "-1"])
    with pytest.raises(SystemExit):
        kin.main(["--pileup", "x", "--out", str(tmp_path / "o"), "--min-snp", "-3"])
    assert kin.main(["--pileup", str(tmp_path / "none.pileup.txt"), "--out", str(tmp_path / "o")]) == 2
    assert "none.pileup.txt" in capsys.readouterr().err
    (tmp_path / "bad.pileup.txt").write_text("WHAT\t1\n")
    assert kin.main(["--pileup", str(tmp_path / "bad.pileup.txt"), "--out", str(tmp_path / "o")]) == 2
    (tmp_path / "e.pileup.txt").write_text("NV\t0\nNSNP\t0\nNCELL\t0\n")
    assert kin.main(["--pileup", str(tmp_path / "e.pileup.txt"), "--out", str(tmp_path / "o")]) == 2
    assert "no genotype columns" in capsys.readouterr().err
    assert not list(tmp_path.glob("o.*"))
