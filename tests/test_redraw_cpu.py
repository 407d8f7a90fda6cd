"""CPU: the contract of the model-drawn null pool (tests/redraw_ref.py, the restatement the GPU is compared with) and
demuxlet_amd/redraw.py's host side.

The hash streams, the genotype rule, the threshold rule, and the law itself: on a PAIR-mode redraw of a pool of 320 barcodes the
goodness-of-fit statistic of tests/fit_ref.py and the first reads' ALT counts are standard normal, so |T| < 4.5 is a 7e-6 tail; the same
redraw with p_c and 1 - p_c exchanged must miss that bound.  Measured once with the seeds of redraw_ref.law_pool (47 263 pairs, 75 532
reads): fit T = -0.23, first reads T = -1.56 directed and -0.82 plain; exchanged: -225, -197 and +3.97 (the plain sum cancels between
REF- and ALT-leaning pairs, which is why redraw_ref.first_read_T has the directed form and the exchange is judged by that one).

Error 0.75 belongs to base qualities 0 and 1 under the engine's own tables (dmx_phred_tables); quality 2 has 10^-0.2 there.  The rule "error
0.75 gives q = 0.5" is checked on the engine's tables at 0 and 1 and, for qualities 0, 1 and 2, on tables that put 0.75 at all three."""
import math

import numpy as np
import pytest

import fit_ref as F
import redraw_ref as R
from compose_ref import GOLD, M64


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import build, capi, engine, redraw, synth
    build.build()
    capi.load()
    mat, err = engine.phred_tables()
    return dict(engine=engine, synth=synth, redraw=redraw, mat=mat, err=err)


# ---- hash streams ---------------------------------------------------------------------------------------------------------------------

def test_streams_of_a_barcode_never_share_a_first_level_key():
    """The read stream and the two PAIR genotype streams of barcode id take seed + GOLD k at k = 4 id + 1, + 2, + 3: three different
    multiples of an odd constant (mod 2^64 the map k -> GOLD k is a bijection), and no two barcodes share a k."""
    assert GOLD % 2 == 1
    seen = {}
    for cid in list(range(200)) + [2 ** 31 - 1, 2 ** 40 + 7]:
        for what, k in (("read", 4 * cid + 1), ("g0", 4 * cid + 2), ("g1", 4 * cid + 3)):
            assert k not in seen, (seen.get(k), cid, what)
            seen[k] = (cid, what)
    for seed in (0, 1, 2 ** 63 + 5):
        for cid in (0, 1, 77, 2 ** 33):
            keys = {R.read_key(seed, cid), R.geno_key(R.PAIR, seed, 0, cid, 0, 3), R.geno_key(R.PAIR, seed, 0, cid, 1, 3)}
            pre = {(seed + GOLD * (4 * cid + k)) & M64 for k in (1, 2, 3)}
            assert len(keys) == 3 and len(pre) == 3


def test_donor_keys_ignore_seed_barcode_and_slot():
    for v in (0, 1, 5, 1023):
        ks = {R.geno_key(R.DONOR, seed, 42, cid, slot, v) for seed in (0, 9, 2 ** 60) for cid in (0, 3, 10 ** 6) for slot in (0, 1)}
        assert len(ks) == 1
        assert R.geno_key(R.DONOR, 0, 43, 0, 0, v) not in ks                   # geno_seed does reach it
        assert R.geno_key(R.DONOR, 0, 42, 0, 0, v + 1) not in ks               # and the sample


def test_uniform_is_32_bits_and_keyed_by_snp_and_read():
    k = R.read_key(5, 11)
    u = [R.uniform32(k, snp, r) for snp in (0, 1, 2 ** 31 - 2) for r in (0, 1, 299)]
    assert all(0 <= x < 2 ** 32 for x in u) and len(set(u)) == len(u)


# ---- genotype rule --------------------------------------------------------------------------------------------------------------------

SUB = float(np.float32(1e-45))                     # the smallest float32 subnormal
UGS = (0, 1, 2 ** 31, 2 ** 32 - 1)


def test_a_zero_weight_genotype_is_never_drawn():
    vals = (0.0, SUB, float(np.float32(1e-40)), 1e-6, 0.25, 1.0, float(np.float32(3.4e38)))
    n = 0
    for w0 in vals:
        for w1 in vals:
            for w2 in vals:
                row = np.array([w0, w1, w2], dtype=np.float32)
                if not R.row_ok(row):
                    assert w0 == w1 == w2 == 0.0
                    continue
                for ug in UGS + (12345, 2 ** 32 - 2):
                    gdraw = R.genotype_of(row, ug)
                    assert row[gdraw] != 0.0, (row, ug, gdraw)
                    n += 1
    assert n > 2000


def test_genotype_rule_edges():
    one_hot = np.eye(3, dtype=np.float32)
    for k in range(3):
        assert all(R.genotype_of(one_hot[k], ug) == k for ug in UGS)
    sub = np.array([SUB, 0.0, SUB], dtype=np.float32)                            # a subnormal row: halves at ug = 2^31
    assert [R.genotype_of(sub, ug) for ug in UGS] == [0, 0, 2, 2]
    thirds = np.array([1.0, 1.0, 1.0], dtype=np.float32)
    assert [R.genotype_of(thirds, ug) for ug in (0, 2 ** 32 // 3, 2 ** 32 // 3 + 1, 2 ** 32 - 1)] == [0, 0, 1, 2]
    for bad in ([0, 0, 0], [1, -0.5, 1], [np.nan, 1, 1], [np.inf, 0, 0]):
        assert not R.row_ok(np.array(bad, dtype=np.float32))


# ---- threshold rule -------------------------------------------------------------------------------------------------------------------

def test_threshold_rule(m):
    assert R.threshold(0.0) == 0 and R.threshold(1.0) == 2 ** 32                 # u < 0 never; every u < 2^32
    assert all(not (u < R.threshold(0.0)) and u < R.threshold(1.0) for u in UGS)
    assert R.threshold(0.5) == 2 ** 31 and R.threshold(1.0 - 2.0 ** -53) == 2 ** 32 - 1
    for bad in (-1e-300, 1.0 + 2.0 ** -52, math.nan, math.inf):
        assert R.threshold(bad) is None
    mat, e3 = m["mat"], m["err"] / 3.0
    ps = (0.0, 1.0, 0.5, 0.1, 0.3, 1.0 / 3.0, 0.7 * 0.5 + 0.3 * 0.123, 1e-17, 1.0 - 2.0 ** -53)
    assert m["err"][0] == m["err"][1] == 0.75 and m["err"][2] != 0.75
    for bq in (0, 1):                                                            # the engine's tables: error 0.75 at 0 and 1
        assert all(R.alt_probability(p, mat[bq], e3[bq]) == 0.5 for p in ps)
    mat2, err2 = m["mat"].copy(), m["err"].copy()
    mat2[:3], err2[:3] = 0.25, 0.75                                              # tables with error 0.75 at 0, 1 and 2
    for bq in (0, 1, 2):
        assert all(R.alt_probability(p, mat2[bq], err2[bq] / 3.0) == 0.5 for p in ps)
    # a hard genotype: q is the read's error (REF hom) or its complement (ALT hom), and sums to 1 over the two alleles' roles
    for bq in (13, 40, 93, 127):
        q0, q2 = R.alt_probability(0.0, mat[bq], e3[bq]), R.alt_probability(1.0, mat[bq], e3[bq])
        assert 0.0 < q0 < 0.5 < q2 < 1.0 and abs(q0 + q2 - 1.0) < 1e-15


def test_restatement_structure_and_counts(m):
    """Low 7 bits kept; unused barcodes, skipped pairs and allele-2-only pairs unchanged with geno -1; the counts add up."""
    rng = np.random.default_rng(5)
    S, V, B = 60, 4, 14
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = np.stack([m["engine"].geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    g[3, 1] = 0.0; g[9, 0] = (1.0, -1.0, 0.5); g[11, 2] = (np.nan, 0.2, 0.2); g[5, :] = (0.0, 1.0, 0.0)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.6, 2.5, doublet_rate=0.5, quals="full")
    hyp = sp.truth.copy(); hyp[2] = (-1, -1); hyp[7] = (-1, 2)
    alpha = np.where(hyp[:, 1] >= 0, 0.37, 0.0)
    rho = rng.choice([0.0, 0.3, 1.0], size=B); a = rng.uniform(0, 1, size=S)
    for mode in (R.PAIR, R.DONOR):
        r = R.redraw(sp, hyp, alpha, rho, a, g, m["mat"], m["err"], 7, 8, mode)
        assert np.array_equal(r["reads"] & 127, sp.reads & 127)
        cell, snp, nrd, start, _ = F.host_pairs(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd)
        drawn = r["geno"][:, 0] >= 0
        assert (nrd == 0).any() and not drawn[nrd == 0].any() and not drawn[hyp[cell, 0] < 0].any()
        bad = (snp == 3) & (hyp[cell] == 1).any(axis=1) | (snp == 9) & (hyp[cell] == 0).any(axis=1) | (snp == 11) & (hyp[cell] == 2).any(axis=1)
        used = (hyp[cell, 0] >= 0) & (nrd > 0)
        assert (bad & used).sum() == r["n_pairs_skipped"] > 0 and not drawn[bad].any() and drawn[used & ~bad].all()
        assert r["n_pairs_drawn"] == int(drawn.sum()) and r["n_reads_drawn"] + r["n_reads_kept"] == int(nrd[drawn].sum())
        same = np.ones(len(sp.reads), dtype=bool)
        for p in np.flatnonzero(drawn):
            same[start[p]:start[p] + nrd[p]] = False
        assert np.array_equal(r["reads"][same], sp.reads[same]) and (r["reads"] != sp.reads).any()
        assert ((r["geno"][:, 1] >= 0) == (drawn & (hyp[cell, 1] >= 0))).all()
        assert (r["geno"][drawn & (snp == 5)] <= 1).all() and (r["geno"][drawn & (snp == 5), 0] == 1).all()    # the one-hot row
        if mode == R.DONOR:                                                      # one genotype per (SNP, sample)
            seen = {}
            for p in np.flatnonzero(drawn):
                for s in range(2):
                    v = hyp[cell[p], s]
                    if v >= 0:
                        assert seen.setdefault((snp[p], v), r["geno"][p, s]) == r["geno"][p, s]
            assert len(seen) > 50


# ---- the law --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def law(m):
    sp, g, hyp, alpha, rho, a = R.law_pool(m["synth"], m["engine"].geno_from_gt)
    idx, prob = R.marginal_first_read(sp, hyp, alpha, rho, a, g, m["mat"], m["err"])
    return dict(sp=sp, g=g, hyp=hyp, alpha=alpha, rho=rho, a=a, idx=idx, prob=prob)


def law_statistics(m, law, swap):
    sp, g, hyp, alpha, rho, a = (law[k] for k in ("sp", "g", "hyp", "alpha", "rho", "a"))
    r = R.redraw(sp, hyp, alpha, rho, a, g, m["mat"], m["err"], R.LAW_SEED, R.LAW_GENO_SEED, R.PAIR, swap=swap)
    f = F.ref_fit(sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, r["reads"], hyp, alpha, rho, a, g, 4, m["mat"], m["err"])
    first = [R.first_read_T(sp, r["reads"], law["idx"], law["prob"], directed=d) for d in (True, False)]
    return R.fit_T(f, hyp[:, 0] >= 0), first, r


def test_the_redrawn_pool_obeys_the_law(m, law):
    sp, hyp, rho = law["sp"], law["hyp"], law["rho"]
    assert sp.n_cells >= 300 and 120 < np.diff(sp.cell_pair_off).mean() < 180
    assert (hyp[:, 1] >= 0).sum() > 80 and (hyp[:, 1] < 0).sum() > 80 and set(rho.tolist()) == {0.0, 0.2}
    t_fit, t_first, r = law_statistics(m, law, swap=False)
    print(f"fit T = {t_fit:+.3f}, first-read T = {t_first[0]:+.3f} (directed) {t_first[1]:+.3f} (plain) over {len(law['idx'])} pairs; "
          f"{r['n_reads_drawn']} reads drawn")
    assert r["n_reads_kept"] == 0 and r["n_pairs_skipped"] == 0 and r["n_pairs_drawn"] == len(law["idx"])
    assert abs(t_fit) < 4.5, t_fit
    assert abs(t_first[0]) < 4.5 and abs(t_first[1]) < 4.5, t_first


def test_the_bound_can_fail(m, law):
    """The same redraw with p_c and 1 - p_c exchanged is not a draw from the law: the fit statistic and the directed first-read statistic
    must miss the bound (the plain first-read sum cancels between REF- and ALT-leaning pairs and is not asked)."""
    t_fit, t_first, _ = law_statistics(m, law, swap=True)
    print(f"exchanged: fit T = {t_fit:+.3f}, first-read T = {t_first[0]:+.3f} (directed) {t_first[1]:+.3f} (plain)")
    assert not abs(t_fit) < 4.5
    assert not abs(t_first[0]) < 4.5


# ---- redraw.py's pure functions --------------------------------------------------------------------------------------------------------

def test_p_emp(m):
    D = m["redraw"]
    null = np.array([[0.0, 1.0, np.nan, -30.0], [1.0, 1.0, 2.0, -31.0], [2.0, -1.0, 3.0, np.nan], [3.0, 0.5, 4.0, -29.0], [4.0, 0.0, 5.0, -28.0]])
    p = D.p_emp(np.array([2.0, -50.0, 10.0, np.nan]), null)
    assert p[0] == 4.0 / 6.0 and p[1] == 1.0 / 6.0 and p[2] == 5.0 / 6.0 and np.isnan(p[3])       # <= counts the tie; nan never counts
    mean, sd = D.null_moments(null)
    assert mean[0] == 2.0 and abs(sd[0] - math.sqrt(2.0)) < 1e-15 and mean[2] == 3.5 and abs(mean[3] + 29.5) < 1e-12
    assert np.isnan(D.null_moments(np.full((2, 1), np.nan))[0][0])
    pooled = D.pooled_null(np.array([[0.0, 1.0, np.nan], [2.0, 3.0, np.inf]]), 0.5)
    assert pooled == dict(n=4, mean=1.5, sd=math.sqrt(1.25), quantile=1.5)
    assert D.pooled_null(np.array([np.nan]), 0.1)["n"] == 0


def test_summary_counts(m):
    D = m["redraw"]
    hyp = np.array([[0, -1], [0, -1], [0, -1], [0, -1], [1, 2], [1, 2], [1, 2], [1, 2], [1, 2], [-1, -1]])
    best = ["SNG-a", "SNG-b", "DBL-a-b-0.5", "AMB-a-b-c", "DBL-b-c-0.5", "DBL-c-b-0.5", "DBL-a-b-0.5", "SNG-b", "", "SNG-a"]
    sng1 = np.array([0, 1, 0, 0, 1, 2, 0, 1, -1, 0])
    dbl1 = np.array([0, 1, 0, 0, 1, 2, 0, 1, -1, 0])
    dbl2 = np.array([1, 2, 1, 1, 2, 1, 1, 2, -1, 1])
    c = D.summary_counts(hyp, best, sng1, dbl1, dbl2)
    assert c["SNG"] == dict(n=4, n_ok=1, as_dbl=1, as_sng=0, wrong=1, amb=1)
    assert c["DBL"] == dict(n=5, n_ok=2, as_dbl=0, as_sng=1, wrong=1, amb=1)
    tot = {k: dict(n=0, n_ok=0, as_dbl=0, as_sng=0, wrong=0, amb=0) for k in ("SNG", "DBL")}
    D.add_counts(tot, c); D.add_counts(tot, c)
    assert tot["DBL"]["n"] == 10 and tot["SNG"]["wrong"] == 2
    assert D.truth_ok(1, 2, "DBL-c-b-0.5", 2, 2, 1) and not D.truth_ok(1, 2, "", -1, -1, -1) and not D.truth_ok(0, -1, "SNG-b", 1, 1, 2)


def test_summary_file(m, tmp_path):
    D = m["redraw"]
    c = {"SNG": dict(n=4, n_ok=1, as_dbl=1, as_sng=0, wrong=1, amb=1), "DBL": dict(n=5, n_ok=2, as_dbl=0, as_sng=1, wrong=1, amb=1)}
    D.write_summary_tsv(str(tmp_path / "s.tsv"), c, dict(n=800, mean=0.0123456, sd=1.01, quantile=-3.2), dict(n=0, mean=np.nan, sd=np.nan, quantile=np.nan), 0.001)
    rows = [l.split("\t") for l in (tmp_path / "s.tsv").read_text().splitlines()]
    assert "\t".join(rows[0]) == D.SUMMARY_HEADER.rstrip("\n") and rows[1] == ["SNG", "4", "1", "1", "0", "1", "1"] and rows[2][0] == "DBL"
    assert "\t".join(rows[3]) == D.POOLED_HEADER.rstrip("\n")
    assert rows[4] == ["#NULL.FIT", "800", "0.012346", "1.010000", "-3.2000", "0.001"] and rows[5][:3] == ["#NULL.SITES", "0", "NA"]


def test_argument_checks(m):
    D = m["redraw"]
    D.check_args(1, 0.001, 0, 1, "pair")
    for bad in (dict(reps=0), dict(fpr=0.0), dict(fpr=1.0), dict(min_cells=-1), dict(max_reads=0), dict(max_reads=9), dict(genotype_draw="cell"),
                dict(seed=-1), dict(geno_seed=-1)):
        kw = dict(reps=5, fpr=0.01, min_cells=10, max_reads=4, genotype_draw="donor", seed=0, geno_seed=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            D.check_args(**kw)
    a = D.parse_args(["--pileup", "x", "--out", "y"])
    assert a.reps == 20 and a.genotype_draw == "donor" and a.max_reads == 4 and a.min_cells == 10 and a.fpr == 0.001 and a.ambient == "reads"
    assert not a.singlets_only and a.seed == 0 and a.geno_seed == 0
    for argv in (["--reps", "0"], ["--fpr", "2"], ["--genotype-draw", "cell"], ["--ambient", "reads"], ["--max-reads", "9"], ["--seed", "-3"]):
        with pytest.raises(SystemExit):
            D.parse_args(["--pileup", "x", "--out", "y"] + argv)


def test_struct_mirrors_match_the_c_compiler(tmp_path):
    import ctypes as C
    import subprocess
    from pathlib import Path
    from demuxlet_amd import capi
    root = Path(__file__).resolve().parents[1]
    rq = ("n_cells", "n_snps", "hyp_memory", "genotype_draw", "hyp", "alpha", "rho", "ambient", "seed", "geno_seed", "index_base", "reserved")
    inf = ("kernel_ms", "bytes_read", "bytes_written", "n_pairs_drawn", "n_pairs_skipped", "n_reads_drawn", "n_reads_kept", "n_cells", "n_used",
           "n_singlet", "n_doublet", "genotype_draw", "reserved")
    assert tuple(n for n, _ in capi.RedrawRequest._fields_) == rq and tuple(n for n, _ in capi.RedrawInfo._fields_) == inf
    exprs = ["sizeof(dmx_redraw_request)"] + [f"offsetof(dmx_redraw_request, {n})" for n in rq]
    exprs += ["sizeof(dmx_redraw_info)"] + [f"offsetof(dmx_redraw_info, {n})" for n in inf]
    exprs += ["(size_t)DMX_REDRAW_PAIR", "(size_t)DMX_REDRAW_DONOR"]
    (tmp_path / "s.c").write_text('#include "dmx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){' +
                                  "".join(f'printf("%zu\\n", {e});' for e in exprs) + "return 0;}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{root / 'include'}", str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = list(map(int, subprocess.check_output([str(tmp_path / "s")], text=True).split()))
    want = [C.sizeof(capi.RedrawRequest)] + [getattr(capi.RedrawRequest, n).offset for n in rq]
    want += [C.sizeof(capi.RedrawInfo)] + [getattr(capi.RedrawInfo, n).offset for n in inf]
    assert got == want + [capi.DMX_REDRAW_PAIR, capi.DMX_REDRAW_DONOR]
    assert capi.RedrawRequest.ambient.offset == capi.FitRequest.ambient.offset
