"""CPU: demuxlet_amd/blocks.py without a GPU — make_blocks, the statistics against the straight loops of tests/blocks_ref.py to the bit,
the leave-one-block-out calls against the oracle's run on the pileup without the block, the three scenarios of tests/blocks_scenarios.py
through the oracle's per-block values, the writers, the command line and the struct mirrors.

Leave-one-out against the oracle: summing block values and subtracting one is not the oracle's sum over the remaining SNPs to the last
bit, so a barcode whose deciding margin under some deletion is within 1e-6 of a threshold is excluded; at most 2 % may be (measured on the
soup scenario, the one with calls near thresholds: 0 of 150)."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import blocks_ref as R
import blocks_scenarios as SC


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import blocks, build, capi, engine, synth
    build.build()
    capi.load()
    return dict(blocks=blocks, engine=engine, synth=synth, capi=capi)


def as_rows(blocks, d):
    return blocks.BestRows(d["best"], d["kind"], d["sng1"], d["sng2"], d["dbl1"], d["dbl2"], d["n_alpha"])


_SCEN = {}


def scen(m, oracle, name):
    """A scenario, the oracle's whole-genome rows and its per-block values: computed once, then read only."""
    if name not in _SCEN:
        sc = SC.scenario(m["engine"], m["synth"], name)
        grid, _ = R.oracle_grid(oracle, sc["pl"], sc["g"], SC.ALPHAS)
        rows = as_rows(m["blocks"], R.best_rows(grid, sc["sample_ids"], SC.ALPHAS))
        extra = m["blocks"].extras_from_rows(rows)
        res = R.block_values(oracle, m["engine"], sc["pl"], sc["g"], SC.ALPHAS, sc["block"], SC.G, extra)
        for a in res.values():
            a.setflags(write=False)
        _SCEN[name] = dict(sc=sc, rows=rows, res=res, grid=grid)
    return _SCEN[name]


# ---- make_blocks
RAGGED = [(3, 10 * i) for i in range(37)] + [(1, 5 + i) for i in range(5)] + [(7, 1000 * i) for i in range(158)] + [(3, 7)] + \
         [(9, 3 * i) for i in range(64)]


def check_blocks(ids, table, snps):
    rid = np.array([s[0] for s in snps])
    assert ids.dtype == np.int32 and len(ids) == len(snps)
    assert np.all(np.diff(ids) >= 0) and np.all(np.diff(ids) <= 1) and ids[0] == 0
    assert np.all(ids[1:][np.diff(rid) != 0] != ids[:-1][np.diff(rid) != 0])             # no block across a change of RID
    assert [t[0] for t in table] == list(range(ids.max() + 1)) and sum(t[4] for t in table) == len(snps)
    for b, r, start, end, n in table:
        sel = np.flatnonzero(ids == b)
        assert n == len(sel) and r == snps[sel[0]][0] and start == snps[sel[0]][1] and end == snps[sel[-1]][1]
        assert len(set(rid[sel])) == 1 and np.all(np.diff(sel) == 1)


def test_make_blocks_on_ragged_chromosomes(m):
    mb = m["blocks"].make_blocks
    S = len(RAGGED)
    runs = [37, 5, 158, 1, 64]
    for N in (1, 5, 40, 1000):
        ids, table = mb(RAGGED, N)
        check_blocks(ids, table, RAGGED)
        want = [min(n, max(1, int(round(N * n / S)))) for n in runs]
        assert len(table) == sum(want)
        for a, n, k in zip(np.concatenate([[0], np.cumsum(runs)[:-1]]), runs, want):
            sizes = np.bincount(ids[a:a + n] - ids[a])
            assert len(sizes) == k and sizes.max() - sizes.min() <= 1                    # equal SNP count, to within one
    ids, table = mb(RAGGED, by_chrom=True)
    check_blocks(ids, table, RAGGED)
    assert [t[4] for t in table] == runs and [t[1] for t in table] == [3, 1, 7, 3, 9]      # RID 3 comes back as a block of its own
    ids, table = mb(RAGGED, block_bp=10000)
    check_blocks(ids, table, RAGGED)
    assert [t[4] for t in table if t[1] == 7] == [10] * 15 + [8] and len(table) == 4 + 16
    ids, table = mb(RAGGED, block_bp=25)
    check_blocks(ids, table, RAGGED)
    assert [t[4] for t in table][:13] == [3, 2] * 6 + [3] and all(t[4] == 1 for t in table if t[1] == 7)
    ids, table = mb([], 40)
    assert len(ids) == 0 and table == []
    for bad in (dict(n_blocks=0), dict(block_bp=0)):
        with pytest.raises(ValueError):
            mb(RAGGED, **bad)


# ---- the statistics against the straight loops, to the bit
def same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("name", ["soup", "swap"])
def test_statistics_are_the_explicit_loops(m, oracle, name):
    s = scen(m, oracle, name)
    blocks, rows, res = m["blocks"], s["rows"], s["res"]
    rd = dict(kind=rows.kind, sng1=rows.sng1, sng2=rows.sng2, dbl1=rows.dbl1, dbl2=rows.dbl2)
    # thin some barcodes so that m < 2, m < min_blocks and uncovered blocks occur
    res = {k: v.copy() for k, v in res.items()}
    for b, keep in ((3, 0), (4, 1), (5, 3), (130, 2)):
        for k in ("col", "ext", "l00"):
            res[k][b, keep:] = 0.0
        res["n_snp"][b, keep:] = 0
    st = blocks.block_calls(res, rows, 5)
    for b in range(len(rows.best)):
        w = R.calls_of(res, rd, b, 5)
        assert st["m"][b] == w["m"] and st["flag"][b] == w["flag"] and st["n_loo_same"][b] == w["n_loo_same"] and st["order"][b] == w["order"], b
        for k in ("llr_sng", "se_sng", "llr_dbl", "se_dbl", "top_share", "loo_min"):
            assert same_float(float(st[k][b]), float(w[k])), (b, k, st[k][b], w[k])
        assert st["top_block"][b] == w["top_block"], b
        for k, d in (("z_sng", ("llr_sng", "se_sng")), ("z_dbl", ("llr_dbl", "se_dbl"))):
            if w[d[1]] > 0:
                assert float(st[k][b]) == w[d[0]] / w[d[1]], (b, k)
        differing = [(x[1], -1 if x[1] == R.DBL else x[2], x[3] if x[1] == R.AMB else -1, 0 if x[1] == R.SNG else x[4]) for x in w["loo"] if not x[5]]
        if not differing:
            assert st["loo_call"][b] is None
        else:
            best_n = max(differing.count(x) for x in differing)
            assert st["loo_call"][b] == next(x for x in differing if differing.count(x) == best_n), b
    assert st["m"][3] == 0 and math.isnan(st["se_sng"][4]) and st["flag"][5] == "LOWN" and st["flag"][130] == "LOWN"
    assert blocks.block_donors(res, rows, 10) == R.donors_of(res, rd, 10)
    assert blocks.block_donors(res, rows, 0) == R.donors_of(res, rd, 0)


def test_singlet_ranks_follow_the_reference_scan(m):
    blocks = m["blocks"]
    rng = np.random.default_rng(3)
    col = rng.integers(-4, 0, size=(500, 6)).astype(np.float64)                          # many ties
    s1, s2 = blocks.rank_singlets(col)
    for b in range(len(col)):
        assert (s1[b], s2[b]) == R.scan_singlets(col[b]), b
    e = rng.integers(-3, 0, size=(200, 2)).astype(np.float64)
    d1, d2 = rng.integers(0, 6, size=200), rng.integers(0, 6, size=200)
    o = blocks.doublet_order(e, d1, d2)
    for b in range(200):
        assert o[b] == R.pick_order(e[b, 0], e[b, 1], d1[b], d2[b])


# ---- leave-one-out calls against the oracle's run without the block
def test_loo_calls_are_the_oracles_calls_without_the_block(m, oracle):
    s = scen(m, oracle, "soup")
    sc, rows, res = s["sc"], s["rows"], s["res"]
    B = sc["pl"].n_cells
    rd = dict(kind=rows.kind, sng1=rows.sng1, sng2=rows.sng2, dbl1=rows.dbl1, dbl2=rows.dbl2)
    mine = [R.calls_of(res, rd, b, 5) for b in range(B)]
    st = m["blocks"].block_calls(res, rows, 5)
    near = np.zeros(B, dtype=bool)
    n_checked = 0
    for g in range(SC.G):
        grid, _ = R.oracle_grid(oracle, R.sub_pileup(m["engine"], sc["pl"], sc["block"] != g), sc["g"], SC.ALPHAS)
        for b in range(B):
            d1, d2, n = int(rows.dbl1[b]), int(rows.dbl2[b]), int(rows.n_alpha[b])
            col = grid[b, :, 0, 0]
            ro = R.pick_order(grid[b, d1, d2, n], grid[b, d2, d1, n], d1, d2)
            jb, kb = (d1, d2) if ro == 0 else (d2, d1)
            if min(R.rule_margins(col, grid[b, jb, kb, n], jb, kb)) <= 1e-6:
                near[b] = True
                continue
            kind, r1, r2 = R.rule(col, grid[b, jb, kb, n], jb, kb)
            got = next(x for x in mine[b]["loo"] if x[0] == g)
            assert got[1] == kind, (b, g, got, kind)
            if kind == R.SNG:                                                            # (its margin of 2 makes SNG.1ST unique)
                assert got[2] == r1, (b, g)
            n_checked += 1
    print("excluded", int(near.sum()), "of", B, "checked", n_checked)
    assert near.sum() <= 0.02 * B
    # and the vectorised statistics agree with the loops on what they count
    for b in np.flatnonzero(~near):
        assert st["n_loo_same"][b] == mine[b]["n_loo_same"]


# ---- the three scenarios through the reference's values
@pytest.mark.parametrize("name", ["clean", "soup", "swap"])
def test_scenarios_through_the_reference(m, oracle, name):
    s = scen(m, oracle, name)
    blocks, sc, rows = m["blocks"], s["sc"], s["rows"]
    st = blocks.block_calls(s["res"], rows, 5)
    donors = blocks.block_donors(s["res"], rows, 10)
    labels = [blocks.loo_label(rows, b, st["loo_call"][b], SC.ALPHAS, sc["sample_ids"]) for b in range(sc["pl"].n_cells)]
    print(name, SC.check_outcome(name, sc, rows.kind, rows.sng1, st, labels, donors))
    n_pairs = np.diff(sc["pl"].cell_pair_off)
    assert 130 < n_pairs[SC.SOUP_CELLS:].mean() < 170 and np.array_equal(s["res"]["n_snp"].sum(axis=1), n_pairs)


# ---- writers, the `.best` reader, the command line, the struct mirrors
def test_writers_and_the_best_reader(m, tmp_path):
    blocks = m["blocks"]
    sm, bc = ["a", "b-1", "c"], ["TTT", "AAA", "CCC", "GGG"]
    head = "BARCODE\tRD.TOTL\tBEST\tSNG.1ST\tSNG.LLK1\tSNG.2ND\tSNG.LLK2\tSNG.LLK0\tDBL.1ST\tDBL.2ND\tALPHA\tLLK12\n"
    (tmp_path / "x.best").write_text(head + "AAA\t5\tSNG-b-1\tb-1\t-1.0\ta\t-9.0\t-9\tb-1\tc\t0.500\t-3.0\n"
                                     "TTT\t5\tDBL-c-a-0.500\tc\t-9.0\ta\t-9.5\t-9\tc\ta\t0.500\t-3.0\n"
                                     "GGG\t5\tAMB-a-c-a/c\ta\t-1.0\tc\t-1.5\t-9\ta\tc\t0.250\t-3.0\n")
    rows = blocks.read_best_rows(str(tmp_path / "x.best"), sm, bc, (0.0, 0.25, 0.5))
    assert rows.kind.tolist() == [1, 0, -1, 2] and rows.sng1.tolist() == [2, 1, -1, 0] and rows.sng2.tolist() == [0, 0, -1, 2]
    assert rows.dbl1.tolist() == [2, 1, -1, 0] and rows.dbl2.tolist() == [0, 2, -1, 2] and rows.n_alpha.tolist() == [2, 2, 0, 1]
    assert blocks.extras_from_rows(rows).tolist() == [[[2, 0, 2], [0, 2, 2]], [[1, 2, 2], [2, 1, 2]], [[-1, 0, 0], [-1, 0, 0]], [[0, 2, 1], [2, 0, 1]]]
    with pytest.raises(ValueError):
        blocks.read_best_rows(str(tmp_path / "x.best"), sm, bc, (0.0, 0.3))                # ALPHA off the grid
    with pytest.raises(ValueError):
        blocks.read_best_rows(str(tmp_path / "x.best"), sm, bc[:3], (0.0, 0.25, 0.5))      # a barcode of another job
    nan = math.nan
    st = dict(m=np.array([3, 1, 0, 6]), llr_sng=np.array([0.5, 8.0, nan, 0.25]), se_sng=np.array([1.0, nan, nan, 0.5]),
              z_sng=np.array([0.5, nan, nan, 0.5]), llr_dbl=np.array([6.0, -5.0, nan, -1.0]), se_dbl=np.array([2.0, nan, nan, 1.0]),
              z_dbl=np.array([3.0, nan, nan, -1.0]), top_block=np.array([2, 0, -1, 4]), top_share=np.array([1.5, 1.0, nan, 0.125]),
              loo_min=np.array([-3.0, 0.0, nan, 0.125]), n_loo_same=np.array([2, 1, 0, 5]),
              loo_call=[(0, 2, -1, 0), None, None, (1, -1, -1, 1)], flag=np.array(["LOWN", "LOWN", "LOWN", "FRAGILE"]))
    n = blocks.write_calls_tsv(str(tmp_path / "o.block_calls.tsv"), bc, sm, (0.0, 0.25, 0.5), rows, st)
    lines = (tmp_path / "o.block_calls.tsv").read_text().splitlines()
    assert n == dict(LOWN=2, FRAGILE=1, STABLE=0) and lines[0] + "\n" == blocks.CALLS_HEADER and len(blocks.CALLS_HEADER.split("\t")) == 15
    assert [x.split("\t")[0] for x in lines[1:]] == ["AAA", "GGG", "TTT"]                 # byte-wise barcode order; CCC has no row
    assert lines[1].split("\t") == ["AAA", "SNG-b-1", "1", "8.0000", "NA", "NA", "-5.0000", "NA", "NA", "0", "1.0000", "0.0000", "1", ".", "LOWN"]
    assert lines[2].split("\t") == ["GGG", "AMB-a-c-a/c", "6", "0.2500", "0.5000", "0.500", "-1.0000", "1.0000", "-1.000", "4", "0.1250", "0.1250",
                                    "5", "DBL-c-a-0.250", "FRAGILE"]
    assert lines[3].split("\t")[9:] == ["2", "1.5000", "-3.0000", "2", "SNG-c", "LOWN"]
    k = blocks.write_donors_tsv(str(tmp_path / "o.block_donors.tsv"), sm, [(0, 3, 12, 40, -2.5, 7, 2, "SWAP?"), (1, 0, 2, 3, 1.0, 0, -1, ".")])
    assert k == 1 and (tmp_path / "o.block_donors.tsv").read_text() == blocks.DONORS_HEADER + "a\t3\t12\t40\t-2.5000\t7\tc\tSWAP?\nb-1\t0\t2\t3\t1.0000\t0\t.\t.\n"
    blocks.write_blocks_tsv(str(tmp_path / "o.blocks.tsv"), [(0, 1, 5, 90, 7), (1, 2, 3, 3, 1)])
    assert (tmp_path / "o.blocks.tsv").read_text() == blocks.BLOCKS_HEADER + "0\t1\t5\t90\t7\n1\t2\t3\t3\t1\n"


def test_command_line_parsing(m):
    blocks = m["blocks"]
    a = blocks.parse_args(["--pileup", "x.txt", "--out", "o"])
    assert (a.best, a.blocks, a.block_bp, a.by_chrom, a.min_blocks, a.min_cells, a.alpha, a.fast, a.gpu) == (None, 40, None, False, 5, 10, [0.0, 0.5], False, 0)
    a = blocks.parse_args(["--pileup", "x", "--out", "o", "--best", "b", "--block-bp", "1000000", "--min-blocks", "3", "--min-cells", "20", "--alpha", "0",
                           "0.25", "--fast", "--gpu", "1"])
    assert (a.best, a.blocks, a.block_bp, a.by_chrom, a.min_blocks, a.min_cells, a.alpha, a.fast, a.gpu) == ("b", None, 1000000, False, 3, 20, [0.0, 0.25], True, 1)
    a = blocks.parse_args(["--pileup", "x", "--out", "o", "--by-chrom"])
    assert a.by_chrom and a.blocks is None and a.block_bp is None
    assert blocks.parse_args(["--pileup", "x", "--out", "o", "--blocks", "12"]).blocks == 12
    base = ["--pileup", "x", "--out", "o"]
    for bad in (["--out", "o"], ["--pileup", "x"], base + ["--blocks", "0"], base + ["--block-bp", "0"], base + ["--blocks", "3", "--by-chrom"],
                base + ["--blocks", "3", "--block-bp", "5"], base + ["--min-blocks", "-1"], base + ["--min-cells", "-1"]):
        with pytest.raises(SystemExit):
            blocks.parse_args(bad)


def test_struct_mirrors_match_the_c_compiler(m, tmp_path):
    capi = m["capi"]
    root = Path(__file__).resolve().parents[1]
    rq = ("n_cells", "n_snps", "n_blocks", "n_extra", "block", "extra", "extra_memory", "reserved")
    inf = ("kernel_ms", "zero_ms", "result_bytes", "n_entries", "n_cells", "n_samples", "n_alpha", "n_blocks", "n_extra", "reserved")
    assert tuple(n for n, _ in capi.BlockLlkRequest._fields_) == rq and tuple(n for n, _ in capi.BlockLlkInfo._fields_) == inf
    exprs = ["sizeof(dmx_block_llk_request)"] + [f"offsetof(dmx_block_llk_request, {n})" for n in rq]
    exprs += ["sizeof(dmx_block_llk_info)"] + [f"offsetof(dmx_block_llk_info, {n})" for n in inf] + ["DMX_BLOCK_MAX_EXTRA", "DMX_ABI_VERSION"]
    (tmp_path / "s.c").write_text('#include "dmx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){' +
                                  "".join(f'printf("%zu\\n", (size_t)({e}));' for e in exprs) + "return 0;}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{root / 'include'}", str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = list(map(int, subprocess.check_output([str(tmp_path / "s")], text=True).split()))
    want = [C.sizeof(capi.BlockLlkRequest)] + [getattr(capi.BlockLlkRequest, n).offset for n in rq]
    want += [C.sizeof(capi.BlockLlkInfo)] + [getattr(capi.BlockLlkInfo, n).offset for n in inf] + [capi.DMX_BLOCK_MAX_EXTRA, 8]
    assert got == want
    assert {"dmx_engine_block_llk", "dmx_engine_get_block_llk", "dmx_engine_block_llk_info"} <= set(capi.SYMBOLS)
    assert "dmx_blocks.hpp" in {p.name for p in __import__("demuxlet_amd.build", fromlist=["HEADERS"]).HEADERS}
