"""CPU: the pileup composer's semantics (tests/compose_ref.py, the restatement the GPU tests compare against) on hand-written pileups,
its hash against literal values, the kept fraction; demuxlet_amd.simulate's recipe, writers and argument parsing; the C-ABI's
argument checks that need no GPU."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest

import compose_ref as R

ALL = 1 << 32


def pileup(cells, width=1):
    """cells: a list of {snp: [read bytes]} -> a sparse pileup"""
    po, ro, snp, nrd, reads = [0], [0], [], [], []
    for c in cells:
        for s in sorted(c):
            snp.append(s); nrd.append(len(c[s])); reads.extend(c[s])
        po.append(len(snp)); ro.append(len(reads))
    return NS(n_cells=len(cells), cell_pair_off=np.array(po, dtype=np.int64), cell_read_off=np.array(ro, dtype=np.int64),
              pair_snp=np.array(snp, dtype=np.int32), pair_nrd=np.array(nrd, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32}[width]),
              reads=np.array(reads, dtype=np.uint8))


def cells_of(out):
    """the composed pileup back as a list of {snp: [read bytes]}"""
    res = []
    for o in range(out["n_out"]):
        d, r = {}, int(out["cell_read_off"][o])
        for p in range(int(out["cell_pair_off"][o]), int(out["cell_pair_off"][o + 1])):
            n = int(out["pair_nrd"][p])
            d[int(out["pair_snp"][p])] = [int(x) for x in out["reads"][r:r + n]]
            r += n
        assert r == int(out["cell_read_off"][o + 1])
        res.append(d)
    return res


A = {1: [10, 11], 4: [12], 9: [13, 14, 15]}
B_ = {0: [20], 2: [21, 22], 5: [23]}
C_ = {1: [30], 4: [31, 32], 9: [33]}
SRC = pileup([A, B_, C_, {}, {3: [], 7: [40]}])


def test_mix64_is_splitmix64():
    # the first output of SplitMix64 seeded with 0 (Steele, Lea, Flood 2014; the reference value every implementation quotes)
    assert R.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF


def test_hash_literals():
    # u = mix64(mix64(seed + 0x9E3779B97F4A7C15 (2 i + s + 1)) + (n << 32 | r)) >> 32, worked out once from the formula
    assert R.read_hash(0, 0, 0, 0, 0) == 1210155558
    assert R.read_hash(1, 2, 1, 3, 4) == 3937060034
    assert R.read_hash(0xDEADBEEF, 1000000, 0, 123456, 7) == 2153779980
    # the same in numpy's wrapping uint64 arithmetic
    with np.errstate(over="ignore"):
        def mix(z):
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))
        key = mix(np.uint64(1) + np.uint64(0x9E3779B97F4A7C15) * np.uint64(2 * 2 + 1 + 1))
        assert int(mix(key + np.uint64((3 << 32) | 4)) >> np.uint64(32)) == 3937060034


def test_disjoint_and_identical_snp_sets_keep_all():
    out = R.compose(SRC, [[0, 1], [0, 2]], [[ALL, ALL], [ALL, ALL]], seed=5)
    got = cells_of(out)
    assert got[0] == {**A, **B_} and list(got[0]) == sorted(got[0])                     # disjoint: the ascending union
    assert got[1] == {s: A[s] + C_[s] for s in A}                                      # identical: slot 0's reads, then slot 1's
    assert out["nrd_width"] == 1 and out["pair_snp"].dtype == np.int32 and out["cell_pair_off"].dtype == np.int64


def test_empty_parent_one_parent_keep_zero():
    out = R.compose(SRC, [[3, 0], [0, 3], [0, -1], [0, 1], [3, -1]], [[ALL, ALL], [ALL, ALL], [ALL, 0], [0, ALL], [ALL, ALL]], seed=1)
    got = cells_of(out)
    assert got[0] == A and got[1] == A and got[2] == A                                  # an empty parent adds nothing; slot 1 = -1
    assert got[3] == B_                                                                # keep 0 drops every read and pair of slot 0
    assert got[4] == {}
    none = R.compose(SRC, [[0, 1]], [[0, 0]], seed=1)
    assert none["cell_pair_off"].tolist() == [0, 0] and len(none["reads"]) == 0 and len(none["pair_snp"]) == 0


def test_zero_read_pair_is_decided_as_one_read_of_index_zero():
    seed = 11
    assert cells_of(R.compose(SRC, [[4, -1]], [[ALL, 0]], seed))[0] == {3: [], 7: [40]}
    assert cells_of(R.compose(SRC, [[4, -1]], [[0, 0]], seed))[0] == {}
    for o in range(40):                                                                # output id o: both outcomes occur at keep = 2^31
        u3, u7 = R.read_hash(seed, o, 0, 3, 0), R.read_hash(seed, o, 0, 7, 0)
        want = {}
        if u3 < (1 << 31):
            want[3] = []
        if u7 < (1 << 31):
            want[7] = [40]
        assert cells_of(R.compose(SRC, [[4, -1]], [[1 << 31, 0]], seed, index_base=o))[0] == want
    outcomes = {R.read_hash(seed, o, 0, 3, 0) < (1 << 31) for o in range(40)}
    assert outcomes == {True, False}


def test_same_barcode_in_both_slots_hashes_differently():
    # the barcode sits between neighbours of other SNPs and read bytes: an offset that strays into them shows
    big = pileup([{s: [200 + s % 50] * 3 for s in range(0, 200, 3)}, {s: list(range(s % 7 + 1)) for s in range(200)}, {5: [99, 98], 150: [97]}, {}])
    out = cells_of(R.compose(big, [[1, 1]], [[1 << 31, 1 << 31]], seed=3))[0]
    one = cells_of(R.compose(big, [[1, -1]], [[1 << 31, 0]], seed=3))[0]
    two = {}
    for s in range(200):                                                               # slot 1 alone, from the hash
        kept = [r for r in range(s % 7 + 1) if R.read_hash(3, 0, 1, s, r) < (1 << 31)]
        if kept:
            two[s] = kept
    assert one != two
    assert out == {s: one.get(s, []) + two.get(s, []) for s in sorted(set(one) | set(two))}


def test_index_base_and_recipe_rows_are_independent():
    par = [[0, 1], [2, 0], [4, 2], [1, 1]]
    keep = [[1 << 31, 1 << 30], [3 << 30, 1 << 31], [1 << 31, 1 << 31], [1 << 29, ALL]]
    whole = cells_of(R.compose(SRC, par, keep, seed=9, index_base=100))
    for k in range(4):
        assert cells_of(R.compose(SRC, par[k:k + 1], keep[k:k + 1], seed=9, index_base=100 + k))[0] == whole[k]


def test_dense_source_and_width_do_not_matter():
    rng = np.random.default_rng(2)
    S, Bn = 17, 4
    cells = [{s: rng.integers(0, 256, size=rng.integers(0, 4)).tolist() for s in range(S)} for _ in range(Bn)]
    sparse = pileup(cells)
    dense = NS(**{**vars(sparse), "pair_snp": None})
    wide = pileup(cells, width=2)
    par, keep = [[0, 1], [2, 3], [1, -1]], [[1 << 31, 1 << 31], [ALL, 1 << 30], [1 << 31, 0]]
    a, b, c = (R.compose(x, par, keep, seed=4) for x in (sparse, dense, wide))
    for name in ("cell_pair_off", "cell_read_off", "pair_snp", "reads"):
        assert np.array_equal(a[name], b[name]) and np.array_equal(a[name], c[name])
    assert np.array_equal(a["pair_nrd"], b["pair_nrd"]) and np.array_equal(a["pair_nrd"], c["pair_nrd"])
    assert a["nrd_width"] == 1 and c["nrd_width"] == 2 and c["pair_nrd"].dtype == np.uint16


def test_width_one_becomes_two_at_200_plus_200_reads():
    deep = pileup([{2: [7, 8], 6: [9]}, {6: list(range(200))}, {3: [5]}, {6: list(range(50, 250)), 8: [1]}, {6: [4], 9: [3, 2]}])
    out = R.compose(deep, [[1, 3], [1, -1], [0, 4]], [[ALL, ALL], [ALL, 0], [ALL, ALL]], seed=0)
    assert out["nrd_width"] == 2 and out["pair_nrd"].dtype == np.uint16
    assert out["pair_nrd"].tolist() == [400, 1, 200, 2, 2, 2]
    got = cells_of(out)
    assert got[0] == {6: list(range(200)) + list(range(50, 250)), 8: [1]} and got[1] == {6: list(range(200))}
    assert got[2] == {2: [7, 8], 6: [9, 4], 9: [3, 2]}
    assert R.compose(deep, [[1, -1], [0, 4]], [[ALL, 0], [ALL, ALL]], seed=0)["nrd_width"] == 1


@pytest.mark.parametrize("f", [0.5, 0.1])
def test_kept_fraction(f):
    n = 120000
    thr = int(round(f * ALL))
    key = R.slot_key(12345, 7, 1)
    kept = sum((R.mix64(key + ((s << 32) | r)) >> 32) < thr for s in range(n // 4) for r in range(4))
    assert abs(kept - n * f) <= 5.0 * np.sqrt(n * f * (1.0 - f)), (kept, n * f)


# ---- demuxlet_amd.simulate ---------------------------------------------------------------------------------------------------------------

def test_recipe_is_deterministic_and_well_formed():
    from demuxlet_amd import simulate as sim
    rng = np.random.default_rng(0)
    assign = rng.integers(-1, 5, size=300).astype(np.int32)
    assign[assign == 4] = -1
    assign[7] = 4                                       # donor 4 has one parent: it can be in a HET or SNG row, never in a HOM row
    a = sim.draw_recipe(assign, (1.0, 0.25), (0.5, 0.8), 50, seed=3)
    b = sim.draw_recipe(assign, (1.0, 0.25), (0.5, 0.8), 50, seed=3)
    c = sim.draw_recipe(assign, (1.0, 0.25), (0.5, 0.8), 50, seed=4)
    for k in a:
        assert np.array_equal(a[k], b[k])
    assert not np.array_equal(a["parent"], c["parent"])
    assert len(a["kind"]) == 2 * 2 * 3 * 50
    par, don, kind = a["parent"], a["donor"], a["kind"]
    assert (assign[par[:, 0]] == don[:, 0]).all() and (don[:, 0] >= 0).all()
    het, hom, sng = kind == sim.KIND_HET, kind == sim.KIND_HOM, kind == sim.KIND_SNG
    assert (don[het, 0] != don[het, 1]).all() and (assign[par[het, 1]] == don[het, 1]).all()
    assert (don[hom, 0] == don[hom, 1]).all() and (par[hom, 0] != par[hom, 1]).all() and (don[hom, 0] != 4).all()
    assert (par[sng, 1] == -1).all() and (a["keep"][sng, 1] == 0).all()
    assert a["keep"].max() <= ALL                       # fractions are capped at 1: 2 A F = 1.6 at A = 0.8, F = 1
    k = a["keep"][het & (a["depth"] == 1.0) & (a["share"] == 0.8)]
    assert (k[:, 0] == ALL).all() and (k[:, 1] == round(0.4 * ALL)).all()
    k = a["keep"][hom & (a["depth"] == 0.25) & (a["share"] == 0.5)]
    assert (k == round(0.25 * ALL)).all()
    assert (a["keep"][sng & (a["depth"] == 0.25), 0] == ALL // 4).all()
    # order: depth, share, kind
    assert kind[:150].tolist() == [0] * 50 + [1] * 50 + [2] * 50 and (a["depth"][:300] == 1.0).all() and (a["share"][:150] == 0.5).all()
    assert sim.draw_recipe(assign, (1.0,), (0.5,), None, 0)["n"] == min(2000, int((assign >= 0).sum()))
    one = sim.draw_recipe(np.array([0, 0, 0, -1]), (1.0,), (0.5,), 10, 0)        # one donor: no HET rows
    assert set(one["kind"].tolist()) == {sim.KIND_HOM, sim.KIND_SNG}
    with pytest.raises(ValueError):
        sim.draw_recipe(np.array([-1, -1]), (1.0,), (0.5,), 10, 0)
    with pytest.raises(ValueError):
        sim.draw_recipe(assign, (0.0,), (0.5,), 10, 0)
    with pytest.raises(ValueError):
        sim.draw_recipe(assign, (1.0,), (1.0,), 10, 0)


def test_chunks_cover_the_recipe_in_order():
    from demuxlet_amd import simulate as sim
    par = np.array([[0, 1], [2, -1], [1, 1], [0, 2], [4, 0]], dtype=np.int32)
    every = sim.chunk_recipe(SRC, par, 1)
    assert every == [(k, k + 1) for k in range(5)]
    assert sim.chunk_recipe(SRC, par, 1 << 30) == [(0, 5)]
    some = sim.chunk_recipe(SRC, par, 150)
    assert some[0][0] == 0 and some[-1][1] == 5 and all(a[1] == b[0] for a, b in zip(some, some[1:])) and len(some) > 1


BEST_HEAD = ("BARCODE\tRD.TOTL\tRD.PASS\tRD.UNIQ\tN.SNP\tBEST\tSNG.1ST\tSNG.LLK1\tSNG.2ND\tSNG.LLK2\tSNG.LLK0\tDBL.1ST\tDBL.2ND\tALPHA\tLLK12\tLLK1\tLLK2\t"
             "LLK10\tLLK20\tLLK00\tPRB.DBL\tPRB.SNG1\n")


def best_row(bc, best, s1, s2, d1, d2, prb=1.0):
    return f"{bc}\t9\t9\t9\t5\t{best}\t{s1}\t-1.0\t{s2}\t-2.0\t-3.0\t{d1}\t{d2}\t0.5\t-1.0\t-1.0\t-1.0\t-1.0\t-1.0\t-1.0\t0.5\t{prb}\n"


def test_writers_from_a_fabricated_best(tmp_path):
    from demuxlet_amd import ambient, simulate as sim
    sm = ["s0", "s1", "s2"]
    real_bc = ["AAA", "CCC", "GGG", "TTT"]
    rc = dict(kind=np.array([0, 0, 1, 1, 2, 2], dtype=np.int32), depth=np.array([1.0] * 6), share=np.array([0.5] * 6),
              parent=np.array([[0, 1], [1, 2], [0, 3], [0, 3], [2, -1], [1, -1]], dtype=np.int32),
              keep=np.full((6, 2), ALL, dtype=np.uint64), donor=np.array([[0, 1], [1, 2], [0, 0], [0, 0], [2, -1], [1, -1]], dtype=np.int32), n=2)
    names = [sim.sim_name(k) for k in range(6)]
    assert names == sorted(names) and names[1] == "SIM0000001"
    p = tmp_path / "x.sim.best"
    p.write_text(BEST_HEAD + best_row(names[0], "DBL-s1-s0-0.5", "s0", "s1", "s1", "s0")     # right, donors in the other order
                 + best_row(names[1], "SNG-s1", "s1", "s2", "s1", "s2")                     # a missed doublet
                 + best_row(names[2], "SNG-s0", "s0", "s1", "s0", "s1")                     # right
                 + best_row(names[3], "DBL-s0-s1-0.5", "s0", "s1", "s0", "s1")              # a homotypic doublet called DBL
                 + best_row(names[4], "AMB-s2-s2-s0", "s2", "s0", "s2", "s0"))              # AMB; names[5] has no row at all
    rows = ambient.read_best_rows(str(p), sm, names)
    n_snp, n_read = np.arange(6) + 10, np.arange(6) + 20
    ok = sim.write_sim_tsv(str(tmp_path / "x.sim.tsv"), rc, real_bc, sm, n_snp, n_read, rows)
    assert ok.tolist() == [True, False, True, False, False, False]
    lines = (tmp_path / "x.sim.tsv").read_text().splitlines()
    assert lines[0] + "\n" == sim.SIM_HEADER and len(lines) == 7
    assert lines[1].split("\t") == [names[0], "HET", "1", "0.5", "AAA", "CCC", "s0", "s1", "10", "20", "DBL-s1-s0-0.5", "1"]
    assert lines[5].split("\t") == [names[4], "SNG", "1", "0.5", "GGG", "NA", "s2", "NA", "14", "24", "AMB-s2-s2-s0", "0"]
    assert lines[6].split("\t")[10:] == ["NA", "0"]
    table = sim.power_table(rc, rows.best, ok, n_snp, n_read)
    assert [(t["kind"], t["n"], t["n_sng"], t["n_dbl"], t["n_amb"], t["n_ok"]) for t in table] == \
        [("HET", 2, 1, 1, 0, 1), ("HOM", 2, 1, 1, 0, 1), ("SNG", 2, 0, 0, 2, 0)]
    assert table[0]["rate"] == 0.5 and table[0]["med_snp"] == 10.5 and table[2]["med_read"] == 24.5
    assert sim.het_rate_at_full_depth(table) == 0.5
    # the pool estimate: 1 DBL among 4 real rows; donors' call shares (2, 1, 1) / 4 -> heterotypic fraction 1 - 6/16
    rb = tmp_path / "real.best"
    rb.write_text(BEST_HEAD + best_row("AAA", "SNG-s0", "s0", "s1", "s0", "s1") + best_row("CCC", "SNG-s1", "s1", "s0", "s0", "s1")
                  + best_row("GGG", "DBL-s0-s2-0.5", "s0", "s2", "s0", "s2") + best_row("TTT", "SNG-s0", "s0", "s1", "s0", "s1"))
    pool = sim.pool_estimate(ambient.read_best_rows(str(rb), sm, real_bc), np.array([0, 1, 2, 0]), 0.5)
    assert pool["obs_dbl"] == 0.25 and pool["het_frac"] == pytest.approx(1 - 6 / 16) and pool["est_dbl"] == pytest.approx(0.25 / (0.5 * 0.625))
    sim.write_power_tsv(str(tmp_path / "x.power.tsv"), table, pool)
    pw = (tmp_path / "x.power.tsv").read_text().splitlines()
    assert pw[0] + "\n" == sim.POWER_HEADER
    assert pw[1].split("\t") == ["HET", "1", "0.5", "2", "1", "1", "0", "1", "0.5000", "10.5", "20.5"]
    assert pw[2].startswith("#POOL\tOBS.DBL") and pw[3].split("\t") == ["#POOL", "0.2500", "0.5000", "0.6250", "0.8000"]
    assert [x.split("\t")[0] for x in pw[4:]] == ["HOM", "SNG"]
    sim.write_recipe_tsv(str(tmp_path / "x.recipe.tsv"), rc)
    rl = (tmp_path / "x.recipe.tsv").read_text().splitlines()
    assert rl[0] + "\n" == sim.RECIPE_HEADER and rl[5].split("\t") == [names[4], "SNG", "1", "0.5", "2", "-1", str(ALL), str(ALL)]


def test_row_ok_rules():
    from demuxlet_amd import simulate as sim
    assert sim.row_ok(sim.KIND_HET, (2, 5), "DBL-a-b-0.5", 2, 5, 2) and sim.row_ok(sim.KIND_HET, (2, 5), "DBL-a-b-0.5", 2, 2, 5)
    assert not sim.row_ok(sim.KIND_HET, (2, 5), "DBL-a-b-0.5", 2, 2, 4) and not sim.row_ok(sim.KIND_HET, (2, 5), "SNG-a", 2, 2, 5)
    assert not sim.row_ok(sim.KIND_HET, (2, 5), "AMB-a-b-c", 2, 2, 5)
    assert sim.row_ok(sim.KIND_HOM, (3, 3), "SNG-a", 3, 3, 1) and not sim.row_ok(sim.KIND_HOM, (3, 3), "SNG-a", 1, 3, 1)
    assert sim.row_ok(sim.KIND_SNG, (3, -1), "SNG-a", 3, 0, 1) and not sim.row_ok(sim.KIND_SNG, (3, -1), "DBL-a-b-0.5", 3, 3, 1)


def test_argument_parsing():
    from demuxlet_amd import simulate as sim
    a = sim.parse_args(["--pileup", "x.pileup.txt", "--out", "o"])
    assert a.best is None and a.min_prb == 0.99 and a.n is None and a.depth == [1.0, 0.5, 0.25, 0.1] and a.share == [0.5]
    assert a.seed == 0 and a.alpha == [0.0, 0.5] and not a.fast and a.gpu == 0
    a = sim.parse_args(["--pileup", "x", "--out", "o", "--best", "b", "--min-prb", "0.9", "--n", "7", "--depth", "1", "0.2", "--share", "0.3", "0.5",
                        "--seed", "9", "--alpha", "0", "0.25", "0.5", "--fast", "--gpu", "1"])
    assert (a.best, a.min_prb, a.n, a.depth, a.share, a.seed, a.alpha, a.fast, a.gpu) == ("b", 0.9, 7, [1.0, 0.2], [0.3, 0.5], 9, [0.0, 0.25, 0.5], True, 1)
    for bad in (["--depth", "0"], ["--depth", "1.5"], ["--share", "1"], ["--share", "0"], ["--n", "0"], ["--min-prb", "2"], ["--seed", "-1"]):
        with pytest.raises(SystemExit):
            sim.parse_args(["--pileup", "x", "--out", "o"] + bad)
    with pytest.raises(SystemExit):
        sim.parse_args(["--out", "o"])
    assert sim.threshold(0.5) == 1 << 31 and sim.threshold(1.0) == ALL and sim.threshold(1.7) == ALL and sim.threshold(0.0) == 0


# ---- the C-ABI without a GPU -------------------------------------------------------------------------------------------------------------

def test_compose_entry_points_check_their_arguments_without_a_gpu():
    from demuxlet_amd import build, capi
    build.build()
    L = capi.load()
    par = np.array([[0, -1]], dtype=np.int32); keep = np.array([[ALL, 0]], dtype=np.uint64)
    rq = capi.ComposeRequest(1, 0, 0, par.ctypes.data, keep.ctypes.data, 1)
    inf, pl = capi.ComposeInfo(), capi.Pileup()
    assert L.dmx_engine_compose(None, C.byref(rq)) == capi.DMX_ERR_ARG and b"dmx_engine_compose" in L.dmx_last_error()
    assert L.dmx_engine_composed_pileup(None, C.byref(pl)) == capi.DMX_ERR_ARG
    assert L.dmx_engine_get_composed(None, None, None, None, None, None) == capi.DMX_ERR_ARG
    assert L.dmx_engine_compose_info(None, C.byref(inf)) == capi.DMX_ERR_ARG
    # the binding mirrors the header's structs
    assert C.sizeof(capi.ComposeRequest) == 56 and capi.ComposeRequest.seed.offset == 32
    assert C.sizeof(capi.ComposeInfo) == 80 and capi.ComposeInfo.n_out.offset == 56


def test_header_struct_sizes_match_the_binding(tmp_path):
    import subprocess
    from pathlib import Path
    from demuxlet_amd import capi
    root = Path(__file__).resolve().parents[1]
    (tmp_path / "s.c").write_text('#include "dmx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu\\n", '
                                  'sizeof(dmx_compose_request), offsetof(dmx_compose_request, seed), sizeof(dmx_compose_info), '
                                  'offsetof(dmx_compose_info, nrd_width));return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{root / 'include'}", str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    a, b, c, d = map(int, subprocess.check_output([str(tmp_path / "s")], text=True).split())
    assert (a, b, c, d) == (C.sizeof(capi.ComposeRequest), capi.ComposeRequest.seed.offset, C.sizeof(capi.ComposeInfo), capi.ComposeInfo.nrd_width.offset)
