"""CPU: the host side of the genotype refinement (demuxlet_amd/refine.py) — `.best` parsing, the `.pileup.txt` reader, the
`.refined.tsv` writer — and the new C entry points' refusal without an engine / a GPU.  No GPU compute is called."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def mods():
    from demuxlet_amd import build, capi, engine, refine, synth
    build.build()
    capi.load()
    return dict(capi=capi, engine=engine, refine=refine, synth=synth)


BEST_HEAD = ("BARCODE\tRD.TOTL\tRD.PASS\tRD.UNIQ\tN.SNP\tBEST\tSNG.1ST\tSNG.LLK1\tSNG.2ND\tSNG.LLK2\tSNG.LLK0\tDBL.1ST\tDBL.2ND\tALPHA\tLLK12\t"
             "LLK1\tLLK2\tLLK10\tLLK20\tLLK00\tPRB.DBL\tPRB.SNG1\n")


def best_row(bc, best, s1, s2, prb_sng1):
    return f"{bc}\t10\t10\t10\t5\t{best}\t{s1}\t-1.0\t{s2}\t-2.0\t-3.0\t{s1}\t{s2}\t0.500\t-1.5\t-1.0\t-2.0\t-1.1\t-2.1\t-3.0\t0.01\t{prb_sng1}\n"


def test_assignments_from_best(mods, tmp_path):
    refine = mods["refine"]
    samples = ["NA-1", "NA-2", "HG-3-b"]
    barcodes = ["AAAC-1", "AAAG-1", "AACC-1", "AAGG-1", "ACCC-1", "AGGG-1"]
    p = tmp_path / "x.best"
    p.write_text(BEST_HEAD
                 + best_row("AAGG-1", "SNG-HG-3-b", "HG-3-b", "NA-1", 0.99)       # sample id with '-': taken from SNG.1ST
                 + best_row("AAAC-1", "SNG-NA-2", "NA-2", "NA-1", 0.70)
                 + best_row("AACC-1", "DBL-NA-1-NA-2-0.500", "NA-1", "NA-2", 0.10)  # doublet: ignored
                 + best_row("ACCC-1", "AMB-NA-1-NA-2-NA-1/NA-2", "NA-1", "NA-2", 0.50)   # ambiguous: ignored
                 + best_row("AGGG-1", "SNG-NA-1", "NA-1", "HG-3-b", 1.0))
    a = refine.assignments_from_best(str(p), samples, barcodes)
    assert a.dtype == np.int32
    assert a.tolist() == [1, -1, -1, 2, -1, 0]
    b = refine.assignments_from_best(str(p), samples, barcodes, min_prb=0.9)           # PRB.SNG1 threshold
    assert b.tolist() == [-1, -1, -1, 2, -1, 0]
    q = tmp_path / "bad.best"
    q.write_text(BEST_HEAD + best_row("TTTT-1", "SNG-NA-1", "NA-1", "NA-2", 1.0))
    with pytest.raises(ValueError):
        refine.assignments_from_best(str(q), samples, barcodes)


def test_pileup_txt_round_trip(mods, tmp_path):
    refine, synth, engine = mods["refine"], mods["synth"], mods["engine"]
    rng = np.random.default_rng(11)
    S, V, B = 120, 3, 40
    raw = synth.make_raw_genotypes(rng, S, V)
    gp = synth.raw_gp_from_alleles(rng, raw.alleles)
    g = gp / gp.sum(axis=2, keepdims=True)
    sp = synth.make_pileup(rng, raw.alleles, B, 0.1, 1.6)
    pl = engine.HostPileup(B, S, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads, sp.rd_totl, sp.rd_pass, sp.rd_uniq)
    d = refine.PileupDump([f"S-{j}" for j in range(V)], [(j % 3, 1000 + 7 * j, "ACGT"[j % 4], "ACGT"[(j + 1) % 4]) for j in range(S)],
                          g.astype(np.float32), [synth.barcode_name(c) for c in range(B)], pl)
    path = tmp_path / "x.pileup.txt"
    refine.write_pileup_txt(str(path), d)
    e = refine.read_pileup_txt(str(path))
    assert e.sample_ids == d.sample_ids and e.barcodes == d.barcodes and e.snps == d.snps
    assert e.g.dtype == np.float32 and np.array_equal(e.g.view(np.uint32), d.g.view(np.uint32))
    q = e.pileup
    assert (q.n_cells, q.n_snps) == (B, S)
    for name in ("cell_pair_off", "cell_read_off", "pair_snp", "pair_nrd", "reads", "rd_totl", "rd_pass", "rd_uniq"):
        assert np.array_equal(getattr(q, name), getattr(pl, name)), name
    assert q.pair_nrd.dtype == np.uint8


def test_pileup_txt_reads_the_cli_spelling(mods, tmp_path):
    """C's %a spelling of the genotype matrix and a deep pair (u16 read counts)."""
    refine = mods["refine"]
    reads = "".join(f"\t{i % 2}:{20 + i % 7}" for i in range(300))
    txt = ("NV\t2\nNSNP\t2\nNCELL\t2\nSM\ta\nSM\tb-c\n"
           "SNP\t0\t0\t100\tA\tG\t0x1.fffffep-1\t0x1.4f8b58p-17\t0x0p+0\t0x1p-1\t0x1p-2\t0x1p-2\n"
           "SNP\t1\t1\t200\tC\tT\t0x1p+0\t0x0p+0\t0x0p+0\t0x0p+0\t0x0p+0\t0x1p+0\n"
           "CELL\t0\tAAAA-1\t3\t2\t1\n"
           "CELL\t1\tCCCC-1\t400\t300\t300\n"
           "PAIR\t0\t0\n"
           f"PAIR\t1\t300{reads}\n")
    p = tmp_path / "c.pileup.txt"
    p.write_text(txt)
    d = refine.read_pileup_txt(str(p))
    assert d.sample_ids == ["a", "b-c"] and d.snps == [(0, 100, "A", "G"), (1, 200, "C", "T")]
    assert d.g[0, 0, 0] == np.float32(float.fromhex("0x1.fffffep-1")) and d.g[0, 1, 1] == np.float32(0.25)
    pl = d.pileup
    assert pl.cell_pair_off.tolist() == [0, 0, 2] and pl.cell_read_off.tolist() == [0, 0, 300]
    assert pl.pair_nrd.dtype == np.uint16 and pl.pair_nrd.tolist() == [0, 300]
    assert pl.reads[0] == 20 and pl.reads[1] == (1 << 7) | 21


def test_refined_tsv_columns_and_order(mods, tmp_path):
    refine = mods["refine"]
    S, V = 3, 2
    ll = -np.arange(S * V * 3, dtype=np.float64).reshape(S, V, 3) / 7.0
    n_cell = np.array([[0, 2], [1, 0], [3, 4]], dtype=np.int32)
    n_ref = n_cell * 2
    n_alt = n_cell + 1
    gp = np.full((S, V, 3), 1 / 3, dtype=np.float32)
    snps = [(0, 11, "A", "C"), (0, 22, "G", "T"), (2, 33, "T", "A")]
    p = tmp_path / "o.refined.tsv"
    refine.write_refined_tsv(str(p), snps, ["x-1", "y"], ll, n_cell, n_ref, n_alt, gp)
    lines = p.read_text().splitlines()
    assert lines[0].split("\t") == ["RID", "POS", "REF", "ALT", "SM_ID", "N.CELL", "N.REF", "N.ALT", "LLK0", "LLK1", "LLK2", "GP0", "GP1", "GP2"]
    rows = [ln.split("\t") for ln in lines[1:]]
    assert [(r[1], r[4]) for r in rows] == [("11", "y"), ("22", "x-1"), ("33", "x-1"), ("33", "y")]      # N.CELL > 0 only, SNP then sample
    r = rows[0]
    assert r[:8] == ["0", "11", "A", "C", "y", "2", "4", "3"]
    assert [float(x) for x in r[8:11]] == pytest.approx(list(ll[0, 1]), abs=1e-5)
    assert [float(x) for x in r[11:]] == pytest.approx([1 / 3] * 3, rel=1e-5)
    q = tmp_path / "n.refined.tsv"
    refine.write_refined_tsv(str(q), None, ["x-1", "y"], ll, n_cell, n_ref, n_alt, gp)
    assert q.read_text().splitlines()[1].split("\t")[:5] == [".", "0", ".", ".", "y"]


def test_refine_entry_points_fail_loudly(mods):
    """Without an engine the new entry points return a status and say why; without a GPU the Python route fails like every other engine call."""
    capi = mods["capi"]
    L = capi.load()
    a = np.zeros(4, dtype=np.int32)
    g = np.ones((2, 2, 3), dtype=np.float32)
    rq = capi.RefineRequest(4, capi.DMX_MEM_HOST, a.ctypes.data, 2, 0, g.ctypes.data, 1e-3)
    assert L.dmx_engine_refine_genotypes(None, C.byref(rq)) == capi.DMX_ERR_ARG
    assert b"null" in L.dmx_last_error()
    assert L.dmx_engine_get_refined(None, None, None, None, None, None) == capi.DMX_ERR_ARG
    assert b"null" in L.dmx_last_error()
    p = C.c_void_p()
    assert L.dmx_engine_refined_device_ptr(None, C.byref(p)) == capi.DMX_ERR_ARG
    assert L.dmx_engine_refine_info(None, C.byref(capi.RefineInfo())) == capi.DMX_ERR_ARG
    assert C.sizeof(capi.RefineRequest) == 56 and C.sizeof(capi.RefineInfo) == 64


def test_refine_run_fails_loudly_without_gpu(mods, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    refine, synth, engine, capi = mods["refine"], mods["synth"], mods["engine"], mods["capi"]
    rng = np.random.default_rng(3)
    raw = synth.make_raw_genotypes(rng, 50, 2)
    sp = synth.make_pileup(rng, raw.alleles, 6, 0.3, 1.5)
    pl = engine.HostPileup(6, 50, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads, sp.rd_totl, sp.rd_pass, sp.rd_uniq)
    g = np.stack([engine.geno_from_gt(raw.alleles[s], 0.01) for s in range(50)])
    with pytest.raises(capi.DmxError) as ei:
        refine.refine_run(pl, g, ["a", "b"], (0.0, 0.5), str(tmp_path / "o"), rounds=1, barcodes=[f"c{i}" for i in range(6)])
    assert ei.value.code in (capi.DMX_ERR_NOGPU, capi.DMX_ERR_HIP)
    with pytest.raises(capi.DmxError):
        engine.Engine(2)
