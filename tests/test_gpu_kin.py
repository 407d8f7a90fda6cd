"""GPU (-m gpu): joint genotype tables (Engine.geno_compare / dmx_engine_geno_compare, kin.kin_run).

The contract is one ascending chain of fused multiply-adds per entry over individually rounded operands, so the device's table must
EQUAL the host emulator's (tests/kin_emul.cpp) bit for bit: over column counts around the tile kernel's tile and SNP counts around its
chunk (both read from dmx_kin_info), edge rows, NULL / ones / random weights, and the wide block that only large panels select.  Then the
independence properties, no interference with other results, every error code, and kin_run end to end: the pedigree's flags, the
cross-run match, the command line on a `demuxlet --pileup-only` dump, and LLR.AB against the engine's own singlet likelihoods."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import kin_ref as KR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import build, capi, engine, kin, refine, synth
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return dict(torch=torch, capi=capi, engine=engine, kin=kin, refine=refine, synth=synth)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return KR.build(tmp_path_factory.mktemp("kin_emul"))


@pytest.fixture(scope="module")
def eng(m):
    e = m["engine"].Engine(1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def geom(eng):
    eng.geno_compare(np.ones((1, 1, 3), dtype=np.float32))
    inf = eng.geno_compare_info()
    assert inf["tile_a"] >= 2 and inf["tile_b"] >= 2 and inf["chunk_snps"] >= 2
    return inf["tile_a"], inf["tile_b"], inf["chunk_snps"]


def same_bits(a, b):
    return a.shape == b.shape and bool((KR.bits(a) == KR.bits(b)).all())


def weight_of(kind, rng, S):
    return None if kind == 0 else np.ones(S) if kind == 1 else KR.edge_weight(rng, S)


def test_bits_around_tile_and_chunk(eng, emu, geom):
    """36 shapes: every VA and VB of {1, 3, tile - 1, tile, tile + 1, 2 tile + 1} with each other, S cycling through {0, 1, chunk - 1,
    chunk, chunk + 1, 2 chunk + 1} and the weight through NULL, ones (which must also give NULL's bits) and random with zeros and a
    subnormal.  A and B are different matrices, and VA != VB off the diagonal, so a transposed or mirrored write cannot pass."""
    ta, tb, ch = geom
    va_s = [1, 3, ta - 1, ta, ta + 1, 2 * ta + 1]
    vb_s = [1, 3, tb - 1, tb, tb + 1, 2 * tb + 1]
    s_s = [0, 1, ch - 1, ch, ch + 1, 2 * ch + 1]
    rng = np.random.default_rng(11)
    n_call = 0
    for i, VA in enumerate(va_s):
        for j, VB in enumerate(vb_s):
            S, kind = s_s[(i + j) % 6], (i + 2 * j) % 3
            ga, gb, c = KR.edge_matrix(rng, S, VA), KR.edge_matrix(rng, S, VB), weight_of(kind, rng, S)
            want, nva, nvb = emu.compare(ga, gb, c)
            T, na, nb = eng.geno_compare(ga, gb, c)
            n_call += 1
            assert same_bits(T, want), (VA, VB, S, kind)
            assert (na == nva).all() and (nb == nvb).all()
            inf = eng.geno_compare_info()
            assert inf["flop"] == 32 * VA * VB * S and (inf["n_snps"], inf["n_a"], inf["n_b"]) == (S, VA, VB)
            assert inf["n_invalid_a"] == S * VA - nva.sum() and inf["n_invalid_b"] == S * VB - nvb.sum()
            assert (inf["tile_a"], inf["tile_b"], inf["chunk_snps"]) == geom
            if kind == 1:
                T0, _, _ = eng.geno_compare(ga, gb)
                n_call += 1
                assert same_bits(T0, T)
    assert n_call <= 60


def test_bits_of_the_wide_block(eng, emu, geom):
    """A panel wide enough that the tile kernel takes its larger per-thread block (dmx_kin_info reports a larger tile): ragged in both
    directions, a full chunk and a tail; and the entries of one pair equal their bits from a one-column call (the small block)."""
    ta, tb, _ = geom
    rng = np.random.default_rng(12)
    VA, VB = 513, 511
    eng.geno_compare(KR.edge_matrix(rng, 1, VA), KR.edge_matrix(rng, 1, VB))
    S = 2 * eng.geno_compare_info()["chunk_snps"] + 1                              # (the wide block's own chunk)
    ga, gb, c = KR.edge_matrix(rng, S, VA), KR.edge_matrix(rng, S, VB), KR.edge_weight(rng, S)
    T, na, nb = eng.geno_compare(ga, gb, c)
    inf = eng.geno_compare_info()
    assert inf["tile_a"] > ta and inf["tile_b"] > tb and S == 2 * inf["chunk_snps"] + 1
    want, nva, nvb = emu.compare(ga, gb, c)
    assert same_bits(T, want) and (na == nva).all() and (nb == nvb).all()
    for a, b in ((512, 510), (inf["tile_a"], inf["tile_b"] - 1), (0, 0)):
        T1, _, _ = eng.geno_compare(ga[:, a:a + 1], gb[:, b:b + 1], c)
        assert same_bits(T1[0, 0], T[a, b])


@pytest.fixture(scope="module")
def panel(geom):
    ta, tb, ch = geom
    rng = np.random.default_rng(13)
    S, VA, VB = 2 * ch + 1, ta + 1, 2 * tb + 1
    return dict(S=S, VA=VA, VB=VB, ga=KR.edge_matrix(rng, S, VA), gb=KR.edge_matrix(rng, S, VB), c=KR.edge_weight(rng, S))


def test_independence(m, eng, emu, panel):
    ga, gb, c, S, VA, VB = (panel[k] for k in ("ga", "gb", "c", "S", "VA", "VB"))
    T, na, nb = eng.geno_compare(ga, gb, c)
    assert same_bits(T, emu.compare(ga, gb, c)[0])
    # a pair alone
    for a, b in ((VA - 1, VB - 1), (3, 5), (0, VB - 2)):
        T1, _, _ = eng.geno_compare(ga[:, a:a + 1], gb[:, b:b + 1], c)
        assert same_bits(T1[0, 0], T[a, b])
    # a repeat, after another call in between
    T2, na2, nb2 = eng.geno_compare(ga, gb, c)
    assert same_bits(T2, T) and (na2 == na).all() and (nb2 == nb).all()
    # B is A
    Ts, nsa, nsb = eng.geno_compare(ga, None, c)
    Tt, _, _ = eng.geno_compare(ga, ga, c)
    assert same_bits(Ts, Tt) and same_bits(Ts, emu.compare(ga, None, c)[0]) and (nsa == nsb).all()
    assert not same_bits(Ts, np.ascontiguousarray(Ts.transpose(1, 0, 3, 2)))        # the weight sits on the A side
    # the staged matrix
    e = m["engine"].Engine(VA)
    try:
        e.set_genotypes(ga)
        Tg, _, _ = e.geno_compare(None, gb, c)
        assert same_bits(Tg, T)
        Tg2, _, _ = e.geno_compare(weight=c)
        assert same_bits(Tg2, Ts)
    finally:
        e.close()
    # device inputs
    torch = m["torch"]
    da, db, dc = (torch.from_numpy(x).cuda() for x in (ga, gb, c))
    torch.cuda.synchronize()
    Td, nda, ndb = eng.geno_compare(da.data_ptr(), db.data_ptr(), dc.data_ptr(), memory=m["capi"].DMX_MEM_DEVICE, n_snps=S, n_a=VA, n_b=VB)
    assert same_bits(Td, T) and (nda == na).all() and (ndb == nb).all()
    Td0, _, _ = eng.geno_compare(da.data_ptr(), None, None, memory=m["capi"].DMX_MEM_DEVICE, n_snps=S, n_a=VA)
    assert same_bits(Td0, emu.compare(ga)[0])


def test_n_valid_against_numpy(eng, panel):
    g = panel["ga"]
    s = (g[..., 0].astype(np.float64) + g[..., 1]) + g[..., 2]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(s) & (s > 0) & (g >= 0).all(axis=2)
    _, na, nb = eng.geno_compare(g)
    assert (na == ok.sum(axis=0)).all() and (nb == na).all() and 0 < ok.sum() < ok.size


def test_no_interference(m, panel):
    """run()'s results and an ambient profile are the same bytes before and after a compare."""
    synth, engine = m["synth"], m["engine"]
    rng = np.random.default_rng(14)
    V, S, B = 4, 60, 24
    raw = synth.make_raw_genotypes(rng, S, V)
    g = (0.97 * np.eye(3)[raw.alleles.sum(axis=2)] + 0.01).astype(np.float32)
    sp = synth.make_pileup(rng, raw.alleles, B, 0.5, 1.5)
    pl = engine.HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads, sp.rd_totl, sp.rd_pass, sp.rd_uniq)
    e = engine.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        e.run()
        e.ambient_profile(sp.truth[:, 0], np.full(S, 0.3), np.array([0.0, 0.1, 0.4]))

        def snapshot():
            ll = np.zeros((B, 3)); ns = np.zeros(B, dtype=np.int32); nr = np.zeros(B, dtype=np.int32)
            m["capi"].check(e._L.dmx_engine_get_ambient(e._h, ll.ctypes.data, ns.ctypes.data, nr.ctypes.data))
            grid, l00, summ = e.get_doublet()
            return [*e.get_singlet(), grid, l00, summ, ll, ns, nr]

        before = snapshot()
        e.geno_compare(panel["ga"], panel["gb"], panel["c"])
        e.geno_compare()
        for x, y in zip(before, snapshot()):
            assert x.tobytes() == y.tobytes()
    finally:
        e.close()


def test_errors(m, eng, panel):
    capi = m["capi"]
    ga, gb, c, S, VA, VB = (panel[k] for k in ("ga", "gb", "c", "S", "VA", "VB"))
    L = eng._L

    def call(h=None, **kw):
        f = dict(n_snps=S, n_a=VA, n_b=VB, ga=ga.ctypes.data, gb=gb.ctypes.data, weight=c.ctypes.data, g_memory=capi.DMX_MEM_HOST, reserved=0)
        f.update(kw)
        rq = capi.KinRequest(f["n_snps"], f["n_a"], f["n_b"], f["ga"], f["gb"], f["weight"], f["g_memory"], f["reserved"])
        return L.dmx_engine_geno_compare(eng._h if h is None else h, C.byref(rq))

    fresh = m["engine"].Engine(VA)
    try:
        # before any compare
        t = np.zeros(16)
        assert L.dmx_engine_get_geno_compare(fresh._h, t.ctypes.data, None, None) == capi.DMX_ERR_STATE
        assert L.dmx_engine_geno_compare_info(fresh._h, C.byref(capi.KinInfo())) == capi.DMX_ERR_STATE
        # ga = NULL without a staged matrix, then with one of another shape
        assert call(h=fresh._h, ga=None) == capi.DMX_ERR_STATE
        fresh.set_genotypes(ga)
        assert call(h=fresh._h, ga=None, n_snps=S - 1) == capi.DMX_ERR_STATE
        assert call(h=fresh._h, ga=None, n_a=VA - 1, gb=None, n_b=VA - 1) == capi.DMX_ERR_STATE
        assert call(h=fresh._h, ga=None) == 0
    finally:
        fresh.close()
    assert call() == 0
    assert L.dmx_engine_geno_compare(None, C.byref(capi.KinRequest())) == capi.DMX_ERR_ARG
    assert L.dmx_engine_geno_compare(eng._h, None) == capi.DMX_ERR_ARG
    assert L.dmx_engine_geno_compare_info(eng._h, None) == capi.DMX_ERR_ARG
    assert L.dmx_engine_get_geno_compare(None, None, None, None) == capi.DMX_ERR_ARG
    for kw in (dict(n_a=0), dict(n_a=4097), dict(n_b=0), dict(n_b=4097), dict(n_snps=-1), dict(reserved=1), dict(g_memory=2),
               dict(gb=None), dict(gb=None, n_b=VA + 1)):
        assert call(**kw) == capi.DMX_ERR_ARG, kw
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        w = c.copy(); w[S // 2] = bad
        assert call(weight=w.ctypes.data) == capi.DMX_ERR_ARG, bad
        assert "weight" in L.dmx_last_error().decode()
    # the last good result is still there after the failed calls, and -0.0 is a weight of zero
    T, _, _ = eng.geno_compare(ga, gb, c)
    w = c.copy(); w[c == 0] = -0.0
    assert same_bits(eng.geno_compare(ga, gb, w)[0], T)
    # buffers that cannot fit: the check comes before anything is read
    torch = m["torch"]
    d = torch.zeros(16, dtype=torch.float32, device="cuda")
    assert call(n_snps=2 ** 31 - 1, n_a=4096, n_b=4096, ga=d.data_ptr(), gb=d.data_ptr(), weight=None, g_memory=capi.DMX_MEM_DEVICE) == capi.DMX_ERR_NOMEM
    msg = L.dmx_last_error().decode()
    assert "bytes" in msg and "4096" in msg
    inf = capi.KinInfo()
    assert L.dmx_engine_geno_compare_info(eng._h, C.byref(inf)) == 0 and (inf.n_a, inf.n_b) == (VA, VB)   # (a refused call leaves the last result)


def test_pedigree_flags_through_kin_run(m, tmp_path):
    """The CPU test's panel: every pair's FLAG is its band; the unrelated pairs and the two founders carry no relatedness flag; the
    duplicate, whose reads cannot tell it from k1, is also INSEP."""
    kin = m["kin"]
    S = 4000
    g = KR.pedigree(np.random.default_rng(2024), S)
    hist = np.zeros(128); hist[30] = 1.0
    kl = kin.kl_table(*m["engine"].phred_tables(), hist)
    r = kin.kin_run(g, KR.PEDIGREE, str(tmp_path / "p"), weight=np.full(S, 0.5), kl=kl)
    rows = [x.split("\t") for x in (tmp_path / "p.kin.tsv").read_text().splitlines()]
    assert rows[0] == kin.PAIR_HEADER.rstrip("\n").split("\t") and len(rows) == 1 + 8 * 7 // 2
    for t in rows[1:]:
        band = KR.expected_band(t[0], t[1])
        assert t[-1] == ("DUP,INSEP" if band == "DUP" else band), t
        assert int(t[2]) == S
    flags = {(t[0], t[1]): t[-1] for t in rows[1:]}
    assert flags[("A", "B")] == "." and flags[("k1", "dup")] == "DUP,INSEP" and flags[("C", "D")] == "."
    k1, dup = KR.PEDIGREE.index("k1"), KR.PEDIGREE.index("dup")
    assert r["stats"]["KIN"][k1, dup] == 0.5 and r["llr"][k1, dup] == 0.0 and r["llr"][0, 1] > 100
    donors = [x.split("\t") for x in (tmp_path / "p.kin_donors.tsv").read_text().splitlines()]
    assert donors[0] == kin.DONOR_HEADER.rstrip("\n").split("\t") and len(donors) == 9
    by = {t[0]: t for t in donors[1:]}
    assert by["k1"][3] == "dup" and by["dup"][3] == "k1" and by["h"][3] in ("A", "C") and all(int(t[1]) == S for t in donors[1:])
    # below --min-snp nothing else is said
    r2 = kin.kin_run(g[:50], KR.PEDIGREE, str(tmp_path / "q"), weight=np.full(50, 0.5), kl=kl)
    assert set(r2["flags"].values()) == {"LOWN"}


def test_match_recovers_the_permutation(m, tmp_path):
    """Six hard columns against a .refined.tsv of the same donors permuted, with a seventh donor, 30 % of the rows missing and 2 % of
    the genotypes changed (host restatement for this seed: true matches 0.47, every false pair below 0.04): ASSIGN is the permutation
    and the extra column stays unassigned."""
    kin, refine = m["kin"], m["refine"]
    ga, gb, covered, perm = KR.match_problem(np.random.default_rng(31))
    S = ga.shape[0]
    snps = [(1 + i // 2000, 10 + 7 * i, "A", "G") for i in range(S)]
    ids_a, ids_b = [f"CLUST{j}" for j in range(6)], [f"don{j}" for j in range(7)]
    n = covered.astype(np.int64)
    refine.write_refined_tsv(str(tmp_path / "b.refined.tsv"), snps, ids_b, np.zeros((S, 7, 3)), n, n, n, gb)
    kb, got_ids, gbm = kin.load_matrix(str(tmp_path / "b.refined.tsv"))
    assert got_ids == ids_b
    _, ga2, gb2, info = kin.align(kin.snp_keys(snps), ga, kb, gbm)
    assert info["allele_mismatch"] == 0 and info["only_b"] == 0 and info["shared"] == len(kb)
    r = kin.kin_run(ga2, ids_a, str(tmp_path / "m"), gb=gb2, ids_b=ids_b)
    assert r["assign"].tolist() == perm.tolist()
    assert (r["n_valid_b"] == covered.sum(axis=0)).all() and (r["n_valid_a"] == len(ga2)).all()
    rows = [x.split("\t") for x in (tmp_path / "m.kin_match.tsv").read_text().splitlines()]
    assert rows[0] == kin.MATCH_HEADER.rstrip("\n").split("\t") and len(rows) == 7
    extra = ids_b[(set(range(7)) - set(perm.tolist())).pop()]
    for a, t in enumerate(rows[1:]):
        assert t[0] == ids_a[a] and t[1] == ids_b[perm[a]] and t[7] == ids_b[perm[a]] and t[5] != t[1]
        assert extra not in (t[1], t[7])


def test_command_line(m, tmp_path):
    """On a dump written by the `demuxlet` binary's --pileup-only from synthetic SAM / VCF data: audit mode writes both files with one
    row per pair and per donor; match mode against the dump itself assigns every column to itself."""
    import sam_vcf_synth as sv
    kin = m["kin"]
    cli = Path(kin.__file__).resolve().parent / "demuxlet"
    contigs = [("1", 30000), ("2", 20000)]
    samples = ["smC", "smA", "smB", "smD"]
    rng = np.random.default_rng(23)
    recs = sv.make_vcf(rng, contigs, 150, samples, tmp_path / "v.vcf.gz")
    bcs = [f"BC{i:02d}-1" for i in range(25)]
    sv.make_reads(rng, contigs, recs, 4000, bcs, tmp_path / "r.sam", tmp_path / "r.bam")
    subprocess.run([str(cli), "--sam", str(tmp_path / "r.sam"), "--vcf", str(tmp_path / "v.vcf.gz"), "--field", "GT", "--out", str(tmp_path / "o"),
                    "--pileup-only"], check=True, stderr=subprocess.DEVNULL)
    dump = str(tmp_path / "o.pileup.txt")
    d = m["refine"].read_pileup_txt(dump)
    V = len(d.sample_ids)
    assert kin.main(["--pileup", dump, "--out", str(tmp_path / "a"), "--min-snp", "20"]) == 0
    rows = [x.split("\t") for x in (tmp_path / "a.kin.tsv").read_text().splitlines()]
    assert rows[0] == kin.PAIR_HEADER.rstrip("\n").split("\t") and len(rows) == 1 + V * (V - 1) // 2
    assert all(len(t) == 11 and t[0] in d.sample_ids and t[1] in d.sample_ids and t[-1] for t in rows[1:])
    assert all(np.isfinite(float(t[8])) and float(t[8]) >= 0 for t in rows[1:])
    donors = (tmp_path / "a.kin_donors.tsv").read_text().splitlines()
    assert len(donors) == 1 + V and [x.split("\t")[0] for x in donors[1:]] == list(d.sample_ids)
    assert kin.main(["--pileup", dump, "--out", str(tmp_path / "b"), "--against", dump, "--min-snp", "20"]) == 0
    match = [x.split("\t") for x in (tmp_path / "b.kin_match.tsv").read_text().splitlines()]
    assert len(match) == 1 + V and all(t[0] == t[1] == t[7] for t in match[1:])
    assert not (tmp_path / "b.kin.tsv").exists()


def test_llr_against_the_engines_singlet_likelihoods(m, tmp_path):
    """A small pool with one-hot rows: over the cells of donor 0 the engine's own llk(0) - llk(1) (Engine.run's singlet values) has a
    mean that agrees with LLR.AB within 4 standard errors of that mean."""
    synth, engine, kin = m["synth"], m["engine"], m["kin"]
    rng = np.random.default_rng(15)
    V, S, B = 4, 1500, 400
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.eye(3, dtype=np.float32)[raw.alleles.sum(axis=2)]
    sp = synth.make_pileup(rng, raw.alleles, B, 0.1, 1.2, doublet_rate=0.0)
    pl = engine.HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads, sp.rd_totl, sp.rd_pass, sp.rd_uniq)
    r = kin.kin_run(g, [f"d{j}" for j in range(V)], str(tmp_path / "s"), pileup=pl)
    e = engine.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        e.run()
        llk, _ = e.get_singlet()
    finally:
        e.close()
    cells = np.nonzero(sp.truth[:, 0] == 0)[0]
    d = llk[cells, 0] - llk[cells, 1]
    se = d.std(ddof=1) / np.sqrt(len(d))
    print(f"LLR.AB {r['llr'][0, 1]:.4f}, engine mean {d.mean():.4f}, SE {se:.4f}, {len(d)} cells")
    assert len(cells) == 100 and np.isfinite(d).all() and abs(d.mean() - r["llr"][0, 1]) <= 4 * se
