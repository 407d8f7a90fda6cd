"""CPU: the site audit's model (tests/site_ref.py, the restatement the GPU is compared with) and demuxlet_amd/sites.py's host side.

Anchors to fit_ref.ref_fit and to a brute force over per-read conditional probabilities; the summation plan (chunk boundaries move only
rounding; two barcodes without a common SNP may change places without changing a bit); calibration on pools drawn from the model; the
swapped-rows pool over three rounds with the oracle's singlet calls; drop_snps, the writers, the command line, the struct mirrors.

Calibration (M = 4, gp softened by 0.3, seeds 21 / 22 / 23), measured once with the restatement: singlets at 121 cells per SNP, n = 300:
mean +0.030, sd 0.986, min -2.67; singlets at 30 cells per SNP, n = 400: mean -0.002, sd 0.979, min -3.03; doublets at alpha = 0.5,
121 cells per SNP, n = 300: mean +0.010, sd 1.072, min -2.93.  The rule is test_fit_cpu's: |mean| <= 3 / sqrt(n) (0.173 and 0.150), sd
within 1 +- 4.5 / sqrt(2 (n - 1)) (0.184 and 0.159).

Swapped rows (site_ref.swap_pool: the issue's pool with fewer, deeper barcodes — 8 donors, 1 500 SNPs of which 380 swapped, 250 singlets
at delta = 0.1, 1.25 reads per pair; z_min -6, min_cells 10), measured once with the restatement.  With the oracle's argmax singlet
calls (this file): right singlets 0.996 -> 1.000 -> 1.000 -> 1.000 over rounds 0..3; flagged 378 / 378 / 378, none of them clean; 2 of
the 380 swapped SNPs with N.CELL >= 10 stay unflagged.  With the oracle's full BEST calls (what test_gpu_site.py's end-to-end test runs
on the engine; round 0 calls nearly every singlet a doublet): 0.012 -> 0.936 -> 1.000 -> 1.000; flagged 307 / 377 / 378, none clean;
2 of 380 unflagged."""
import numpy as np
import pytest

import fit_ref as F
import quality_mix as Q
import site_ref as R


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import build, capi, engine, synth
    build.build()
    capi.load()
    mat, err = engine.phred_tables()
    return dict(engine=engine, synth=synth, mat=mat, err=err)


def gt_matrix(m, alleles):
    return np.stack([m["engine"].geno_from_gt(alleles[s], 0.01) for s in range(alleles.shape[0])])


def arrays(sp):
    return sp.cell_pair_off, sp.pair_snp, sp.pair_nrd, sp.reads


def site(m, sp, hyp, alpha, g, M, rho=None, a=None, **kw):
    return R.ref_site(*arrays(sp), hyp, alpha, rho, a, g, M, m["mat"], m["err"], **kw)


def mixed_pool(m, seed, B=200, S=120, V=4, delta=0.3):
    """Singlet and doublet hypotheses (more than one chunk of singlets, a partial last chunk in both lists), unused barcodes, hard and
    all-zero rows, soup."""
    rng = np.random.default_rng(seed)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = gt_matrix(m, raw.alleles)
    g[3, :] = np.array([1.0, 0.0, 0.0], dtype=np.float32)
    g[7, 1] = 0.0
    sp = m["synth"].make_pileup(rng, raw.alleles, B, delta, 2.0, doublet_rate=0.3, quals="edges")
    hyp = sp.truth.copy().astype(np.int32)
    hyp[::11] = (-1, -1)
    alpha = np.where(hyp[:, 1] >= 0, rng.choice([0.0, 0.5, 0.37], size=B), 0.0)
    rho = rng.choice([0.0, 0.1, 0.3], size=B)
    a = rng.uniform(0.0, 1.0, size=S)
    return sp, g, hyp, alpha, rho, a


def test_sums_over_snps_are_fit_refs_sums_over_barcodes(m):
    sp, g, hyp, alpha, rho, a = mixed_pool(m, 3)
    sng, dbl = R.listing(hyp)
    assert len(sng) > 64 and len(sng) % 64 and 0 < len(dbl) and len(dbl) % 64
    for M in (1, 4, 5):
        s = site(m, sp, hyp, alpha, g, M, rho, a)
        sl = site(m, sp, hyp, alpha, g, M, rho, a, longdouble=True)
        f = F.ref_fit(*arrays(sp), hyp, alpha, rho, a, g, M, m["mat"], m["err"], longdouble=True)
        tol = 10 * max(R.drift(s, sl), 1e-15)
        for ks, kf in (("obs", "obs"), ("mean", "mean"), ("var", "var")):
            x, y = float(s[ks].astype(np.longdouble).sum()), float(f[kf].sum())
            assert abs(x - y) <= tol * max(1.0, abs(y)) * len(s[ks]), (M, ks, x, y)
        for ks, kf in (("n_cell", "n_snp"), ("n_read", "n_read"), ("n_trunc", "n_trunc"), ("n_zero", "n_zero")):
            assert int(s[ks].sum()) == int(f[kf].sum()), (M, ks)
        assert s["n_cell"].sum() > 1000 and (s["n_alt"] <= s["n_read"]).all() and s["n_alt"].sum() > 0
        cell, snp, nrd, start, _ = F.host_pairs(*arrays(sp)[:3])
        covered = np.bincount(snp[hyp[cell, 0] >= 0], minlength=sp.n_snps) > 0
        for k in R.KEYS:
            assert not np.asarray(s[k])[~covered].any()


def test_alt_excess_matches_per_read_brute_force(m):
    """exc and vexc against per-read conditional probabilities: given component c the reads are independent with
    q_r = Pr(ALT | c, stored) = t_r(c, 1) / (t_r(c, 0) + t_r(c, 1)), so E k = sum_c pi_c sum_r q_r and
    E k^2 = sum_c pi_c (sum_r q_r (1 - q_r) + (sum_r q_r)^2), pi_c = W_c / sum W — no pattern is enumerated."""
    sp, g, hyp, alpha, rho, a = mixed_pool(m, 5, B=60, S=40)
    M = 5
    t = R.pair_terms(*arrays(sp), hyp, alpha, rho, a, g, M, m["mat"], m["err"])
    s = R.ref_site(*arrays(sp), hyp, alpha, rho, a, g, M, m["mat"], m["err"], terms=t)
    cell, snp, nrd, start, _ = F.host_pairs(*arrays(sp)[:3])
    mat, e3 = m["mat"], m["err"] / 3.0
    exc, vexc = np.zeros(sp.n_snps), np.zeros(sp.n_snps)
    kinds = set()
    for k in np.flatnonzero(t["state"] == 1):
        b, i = cell[k], snp[k]
        v1, v2 = hyp[b]
        rd = np.asarray(sp.reads)[start[k]:start[k] + min(nrd[k], M)].astype(np.int64)
        if v2 < 0:
            W, cm = g[i, v1].astype(np.float64), np.array([0.0, 0.5, 1.0])
        else:
            W = np.array([float(g[i, v1, l]) * float(g[i, v2, k_]) for l in range(3) for k_ in range(3)])
            cm = np.array([0.5 * l + (k_ - l) * 0.5 * alpha[b] for l in range(3) for k_ in range(3)])
        p = (1 - rho[b]) * cm + rho[b] * a[i]
        bq = rd & 127
        t0 = mat[bq][:, None] * (1 - p) + e3[bq][:, None] * p
        t1 = e3[bq][:, None] * (1 - p) + mat[bq][:, None] * p
        q = t1 / (t0 + t1)                                                          # [reads][NC]
        post = W * np.prod(t0 + t1, axis=0)                                         # the component's weight given that every read is stored
        pi = post / post.sum()
        ek = float((pi * q.sum(axis=0)).sum())
        ek2 = float((pi * ((q * (1 - q)).sum(axis=0) + q.sum(axis=0) ** 2)).sum())
        kx = int((rd >> 7).sum())
        assert abs(float(t["terms"][3, k]) - (kx - ek)) <= 1e-10, (k, t["terms"][3, k], kx - ek)
        assert abs(float(t["terms"][4, k]) - (ek2 - ek * ek)) <= 1e-10
        exc[i] += kx - ek; vexc[i] += ek2 - ek * ek
        kinds.add((v2 >= 0, len(rd)))
    assert R.scaled_difference(s["exc"], exc) <= 1e-10 and R.scaled_difference(s["vexc"], vexc) <= 1e-10
    for d_ in (False, True):
        assert (d_, 1) in kinds and max(n for x, n in kinds if x == d_) >= 4


def test_chunk_boundaries_move_only_rounding(m):
    sp, g, hyp, alpha, rho, a = mixed_pool(m, 7)
    t = R.pair_terms(*arrays(sp), hyp, alpha, rho, a, g, 4, m["mat"], m["err"])
    tl = R.pair_terms(*arrays(sp), hyp, alpha, rho, a, g, 4, m["mat"], m["err"], longdouble=True)
    base = site(m, sp, hyp, alpha, g, 4, rho, a, terms=t)
    d = R.drift(base, site(m, sp, hyp, alpha, g, 4, rho, a, terms=tl, longdouble=True))
    moved = 0
    for chunk in (1, 7, 63, 65, 1000):
        r = site(m, sp, hyp, alpha, g, 4, rho, a, terms=t, chunk=chunk)
        for k in R.COUNTS:
            assert np.array_equal(r[k], base[k])
        for k in R.FLOATS:
            assert R.scaled_difference(r[k], base[k]) <= 10 * max(d, 1e-15), (chunk, k)
            moved += r[k].tobytes() != base[k].tobytes()
    print(f"chunk sizes 1, 7, 63, 65, 1000 against 64: {moved} of 25 arrays differ in some bit; drift {d:.3g}")


def test_two_barcodes_without_a_common_snp_may_change_places(m):
    sp, g, hyp, alpha, rho, a = mixed_pool(m, 9, B=200, S=400, delta=0.03)
    t = R.pair_terms(*arrays(sp), hyp, alpha, rho, a, g, 4, m["mat"], m["err"])
    base = site(m, sp, hyp, alpha, g, 4, rho, a, terms=t)
    sng, dbl = R.listing(hyp)
    cell, snp, _, _, _ = F.host_pairs(*arrays(sp)[:3])
    sets = {int(b): set(snp[cell == b].tolist()) for b in sng}
    done = 0
    for i in range(len(sng) - 1):
        x, y = int(sng[i]), int(sng[i + 1])
        if sets[x] & sets[y] or (i + 1) % 64 == 0:                               # neighbours inside one chunk, no common SNP
            continue
        sw = sng.copy(); sw[i], sw[i + 1] = y, x
        r = site(m, sp, hyp, alpha, g, 4, rho, a, terms=t, lists=(sw, dbl))
        for k in R.KEYS:
            assert r[k].tobytes() == base[k].tobytes(), (x, y, k)
        done += 1
        if done == 3:
            break
    assert done >= 1


def calibration(m, seed, S, B, delta, doublets):
    rng = np.random.default_rng(seed)
    V = 4
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = np.stack([m["engine"].geno_from_gp(x, 0.01) for x in m["synth"].raw_gp_from_alleles(rng, raw.alleles, soft=0.3)])
    v1 = np.arange(B) % V
    hyp = np.stack([v1, (v1 + 1) % V if doublets else np.full(B, -1)], axis=1).astype(np.int32)
    alpha = np.full(B, 0.5 if doublets else 0.0)
    sp = F.model_drawn_pool(rng, m["synth"], g, B, delta, 1.5, hyp, alpha, M=4)
    r = site(m, sp, hyp, alpha, g, 4)
    return R.zscore(r), R.zalt(r), float(r["n_cell"].mean())


@pytest.mark.parametrize("name,seed,S,B,delta,doublets,cells", [
    ("singlets, 120 cells", 21, 300, 600, 0.2, False, 120), ("singlets, 30 cells", 22, 400, 200, 0.15, False, 30),
    ("doublets, 120 cells", 23, 300, 600, 0.2, True, 120)])
def test_calibration_on_model_drawn_pools(m, name, seed, S, B, delta, doublets, cells):
    z, za, n_cell = calibration(m, seed, S, B, delta, doublets)
    n = len(z)
    print(f"calibration {name}: n {n} cells/SNP {n_cell:.0f} Z mean {z.mean():+.4f} sd {z.std(ddof=1):.4f} min {z.min():+.2f}; "
          f"Z.ALT mean {za.mean():+.4f} sd {za.std(ddof=1):.4f}")
    assert np.isfinite(z).all() and n == S and 0.8 * cells < n_cell < 1.2 * cells
    assert abs(z.mean()) <= 3.0 / np.sqrt(n), z.mean()
    half = 4.5 / np.sqrt(2.0 * (n - 1))
    assert 1.0 - half <= z.std(ddof=1) <= 1.0 + half, z.std(ddof=1)


def test_swapped_rows_over_three_rounds(m, oracle):
    synth = m["synth"]
    sp, g, swapped, truth = R.swap_pool(m["engine"], synth)
    V, S, B = g.shape[1], sp.n_snps, sp.n_cells
    t = np.ones(B, dtype=np.int32)

    def calls(arr):
        po, ps, pn, rd = arr
        ro = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(B), np.diff(po)), weights=np.asarray(pn, dtype=np.int64), minlength=B))])
        q = synth.SynthPileup(B, S, po, ro.astype(np.int64), ps, pn, rd, t, t, t, sp.truth)
        return Q.oracle_run(oracle, q, g, singlet_only=True).llks.argmax(axis=1).astype(np.int32)

    full = arrays(sp)
    call = calls(full)
    rounds = [(float((call == truth).mean()), None, None)]
    for r in range(1, 4):
        hyp = np.stack([call, np.full(B, -1)], axis=1).astype(np.int32)
        res = R.ref_site(*full, hyp, np.zeros(B), None, None, g, R.SWAP_M, m["mat"], m["err"])
        flag = R.flags(res, R.SWAP_Z_MIN, R.SWAP_MIN_CELLS)
        call = calls(R.drop_pairs(full, flag))
        rounds.append((float((call == truth).mean()), flag, res["n_cell"]))
        print(f"round {r}: flagged {int(flag.sum())} (swapped {int((flag & swapped).sum())}, clean {int((flag & ~swapped).sum())}); "
              f"right singlets {rounds[r - 1][0]:.3f} -> {rounds[r][0]:.3f}")
    seen = swapped & (rounds[-1][2] >= R.SWAP_MIN_CELLS)
    print(f"swapped SNPs with N.CELL >= {R.SWAP_MIN_CELLS}: {int(seen.sum())}, unflagged {int((seen & ~rounds[-1][1]).sum())}")
    R.check_swapped_rounds(rounds, swapped, R.SWAP_MIN_CELLS)


# ---- demuxlet_amd/sites.py: the host side ----------------------------------------------------------------------------------------------

def host_pileup(m, sp):
    return m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads,
                                  sp.rd_totl, sp.rd_pass, sp.rd_uniq)


def rebuilt(m, pl, mask):
    """The pileup rebuilt pair by pair from the pairs that survive the mask."""
    po, ro = [0], [0]
    snps, nrds, rds = [], [], []
    r = 0
    for c in range(pl.n_cells):
        for p in range(int(pl.cell_pair_off[c]), int(pl.cell_pair_off[c + 1])):
            i = int(pl.pair_snp[p]) if pl.pair_snp is not None else p - int(pl.cell_pair_off[c])
            n = int(pl.pair_nrd[p])
            if not mask[i]:
                snps.append(i); nrds.append(n); rds.append(np.asarray(pl.reads)[r:r + n])
            r += n
        po.append(len(snps)); ro.append(int(sum(nrds)))
    return np.array(po), np.array(ro), np.array(snps, dtype=np.int32), np.array(nrds), (np.concatenate(rds) if rds else np.zeros(0, dtype=np.uint8))


@pytest.mark.parametrize("dense", [False, True])
def test_drop_snps(m, dense):
    from demuxlet_amd import sites
    rng = np.random.default_rng(31 + dense)
    S, V, B = 60, 3, 25
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 1.0 if dense else 0.3, 2.0, dense_layout=dense, doublet_rate=0.0)
    assert (sp.pair_snp is None) == dense
    pl = host_pileup(m, sp)
    for mask in (np.zeros(S, dtype=bool), rng.random(S) < 0.3, np.ones(S, dtype=bool)):
        out = sites.drop_snps(pl, mask)
        po, ro, snp, nrd, rd = rebuilt(m, pl, mask)
        assert out.n_cells == B and out.n_snps == S and out.pair_snp is not None and out.pair_snp.dtype == np.int32
        assert np.array_equal(out.cell_pair_off, po) and np.array_equal(out.cell_read_off, ro)
        assert np.array_equal(out.pair_snp, snp) and np.array_equal(out.pair_nrd, nrd) and np.array_equal(out.reads, rd)
        assert out.pair_nrd.dtype == np.asarray(pl.pair_nrd).dtype
        for k in ("rd_totl", "rd_pass", "rd_uniq"):
            assert np.array_equal(getattr(out, k), getattr(pl, k))
        if not mask.any():
            assert len(out.pair_nrd) == len(pl.pair_nrd) and np.array_equal(out.reads, pl.reads)
            if not dense:
                assert np.array_equal(out.pair_snp, pl.pair_snp)
    with pytest.raises(ValueError):
        sites.drop_snps(pl, np.zeros(S + 1, dtype=bool))


def test_site_writers(tmp_path):
    from demuxlet_amd import sites
    snps = [(1, 100, "A", "C"), (1, 250, "G", "T"), (2, 7, "C", "G")]
    r = dict(obs=np.array([-40.0, -10.0, 0.0]), mean=np.array([-12.0, -11.0, 0.0]), var=np.array([4.0, 4.0, 0.0]), exc=np.array([6.0, -0.5, 0.0]),
             vexc=np.array([2.25, 1.0, 0.0]), n_cell=np.array([12, 5, 0]), n_read=np.array([15, 6, 0]), n_alt=np.array([9, 1, 0]),
             n_trunc=np.array([1, 0, 0]), n_zero=np.array([0, 2, 0]))
    z, p, za, flag = sites.site_scores(r, -6.0, 10)
    assert z[:2].tolist() == [-14.0, 0.5] and np.isnan(z[2]) and za[:2].tolist() == [4.0, -0.5] and np.isnan(za[2]) and flag.tolist() == [True, False, False]
    assert sites.site_scores(r, -6.0, 13)[3].tolist() == [False, False, False]                      # too few cells
    assert sites.site_scores(r, 1.0, 5)[3].tolist() == [True, True, False]
    n = sites.write_sites_tsv(str(tmp_path / "o.sites.tsv"), snps, r, z, p, za, flag)
    lines = (tmp_path / "o.sites.tsv").read_text().splitlines()
    assert n == 1 and lines[0] == sites.SITES_HEADER.rstrip("\n") and len(lines) == 4 and len(sites.SITES_HEADER.split("\t")) == 18
    assert lines[1].split("\t") == ["1", "100", "A", "C", "12", "15", "9", "1", "0", "-40.00000", "-12.00000", "2.00000", "-14.0000",
                                    lines[1].split("\t")[13], "6.00000", "1.50000", "4.0000", "MISFIT"]
    assert float(lines[1].split("\t")[13]) < 1e-40
    assert lines[2].split("\t")[4:] == ["5", "6", "1", "0", "2", "-10.00000", "-11.00000", "2.00000", "0.5000", "0.6915", "-0.50000", "1.00000", "-0.5000", "."]
    assert lines[3].split("\t")[9:] == ["0.00000", "0.00000", "0.00000", "NA", "NA", "0.00000", "0.00000", "NA", "."]
    sites.write_rounds_tsv(str(tmp_path / "o.sites_rounds.tsv"), [dict(round=1, n_flag=5, n_released=0, n_new=5, n_best_changed=7),
                                                                  dict(round=2, n_flag=4, n_released=2, n_new=1, n_best_changed=0)])
    assert (tmp_path / "o.sites_rounds.tsv").read_text() == sites.ROUNDS_HEADER + "1\t5\t0\t5\t7\n2\t4\t2\t1\t0\n"


def test_hypotheses_singlets_only():
    from demuxlet_amd import fit, sites
    rows = fit.BestHyp(["SNG-a", "DBL-a-b-0.500", ""], np.array([[0, -1], [0, 1], [-1, -1]], dtype=np.int32), np.array([0.0, 0.5, 0.0]),
                       np.array([0, 0, -1], dtype=np.int32))
    h, al = sites.hypotheses(rows, False)
    assert h.tolist() == [[0, -1], [0, 1], [-1, -1]] and al.tolist() == [0.0, 0.5, 0.0]
    h, al = sites.hypotheses(rows, True)
    assert h.tolist() == [[0, -1], [-1, -1], [-1, -1]] and al.tolist() == [0.0, 0.0, 0.0] and rows.hyp[1].tolist() == [0, 1]


def test_command_line_parsing():
    from demuxlet_amd import sites
    a = sites.parse_args(["--pileup", "x.txt", "--out", "o"])
    assert (a.max_reads, a.z_min, a.min_cells, a.rounds, a.best, a.ambient, a.ambient_tsv, a.alpha, a.singlets_only, a.fast, a.gpu) == \
        (4, -6.0, 10, 1, None, "reads", None, [0.0, 0.5], False, False, 0)
    a = sites.parse_args(["--pileup", "x.txt", "--out", "o", "--best", "b", "--rounds", "3", "--max-reads", "8", "--z-min", "-4", "--min-cells", "20",
                          "--singlets-only", "--ambient-tsv", "t", "--ambient", "census", "--alpha", "0", "0.25", "--fast", "--gpu", "1"])
    assert (a.best, a.rounds, a.max_reads, a.z_min, a.min_cells, a.singlets_only, a.ambient_tsv, a.ambient, a.alpha, a.fast, a.gpu) == \
        ("b", 3, 8, -4.0, 20, True, "t", "census", [0.0, 0.25], True, 1)
    base = ["--pileup", "x", "--out", "o"]
    for bad in (["--out", "o"], ["--pileup", "x"], base + ["--max-reads", "0"], base + ["--max-reads", "9"], base + ["--z-min", "nan"],
                base + ["--rounds", "0"], base + ["--min-cells", "-1"], base + ["--ambient", "reads"], base + ["--ambient-tsv", "t", "--ambient", "soup"]):
        with pytest.raises(SystemExit):
            sites.parse_args(bad)


def test_struct_mirrors_match_the_c_compiler(tmp_path):
    import ctypes as C
    import subprocess
    from pathlib import Path
    from demuxlet_amd import capi
    root = Path(__file__).resolve().parents[1]
    rq = ("n_cells", "n_snps", "hyp_memory", "max_reads", "hyp", "alpha", "rho", "ambient", "partial_bytes", "reserved")
    inf = ("kernel_ms", "bytes", "partial_bytes", "n_trunc", "n_zero", "n_chunks", "n_waves", "chunk_cells", "slab_snps", "n_cells", "n_snps",
           "n_used", "n_singlet", "n_doublet", "max_reads", "reserved")
    assert tuple(n for n, _ in capi.SiteFitRequest._fields_) == rq and tuple(n for n, _ in capi.SiteFitInfo._fields_) == inf
    exprs = ["sizeof(dmx_site_fit_request)"] + [f"offsetof(dmx_site_fit_request, {n})" for n in rq]
    exprs += ["sizeof(dmx_site_fit_info)"] + [f"offsetof(dmx_site_fit_info, {n})" for n in inf]
    (tmp_path / "s.c").write_text('#include "dmx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){' +
                                  "".join(f'printf("%zu\\n", {e});' for e in exprs) + "return 0;}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{root / 'include'}", str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = list(map(int, subprocess.check_output([str(tmp_path / "s")], text=True).split()))
    want = [C.sizeof(capi.SiteFitRequest)] + [getattr(capi.SiteFitRequest, n).offset for n in rq]
    want += [C.sizeof(capi.SiteFitInfo)] + [getattr(capi.SiteFitInfo, n).offset for n in inf]
    assert got == want
    assert C.sizeof(capi.SiteFitRequest) == C.sizeof(capi.FitRequest) + 8 and capi.SiteFitRequest.ambient.offset == capi.FitRequest.ambient.offset
