"""CPU: the pieces of bench.py's --dump-outputs that need no GPU — which barcodes are written when the whole output is larger than the
budget, how the arrays land on disk, and the N-rank dump of a full-size gather (injected records) staying within the budget."""
import sys
import types
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _disk_bytes(d):
    return sum(f.stat().st_size for f in Path(d).glob("*.npy"))


def test_dump_columns_are_the_files_written():
    import bench
    from demuxlet_amd import capi
    nf = len(capi.SUMMARY_DTYPE.names) - 1                            # every summary field but the padding
    assert len(bench.summary_fields(capi.SUMMARY_DTYPE)) == nf == 27
    one = bench.dump_columns(32, 2, True, capi.SUMMARY_DTYPE, grid=True)                  # cfg3, one process
    assert sum(one.values()) == 1 + 32 + 1 + 2 + 32 * 32 * 2 + nf and len(one) == 5 + nf and "sing" not in one
    ranks = bench.dump_columns(64, 2, True, capi.SUMMARY_DTYPE, sing=True)                # cfg4, N ranks: the gathered records
    assert sum(ranks.values()) == 1 + 64 + 1 + 64 + 2 + nf and "grid" not in ranks
    assert bench.dump_columns(8, 2, False, capi.SUMMARY_DTYPE, grid=True) == {"barcode_index": 1, "llks": 8, "llk0s": 1}


def test_dump_sample_is_all_barcodes_or_a_fixed_sample_within_the_budget():
    import bench
    from demuxlet_amd import capi
    small = bench.dump_columns(8, 2, False, capi.SUMMARY_DTYPE)
    assert np.array_equal(bench.dump_sample(1000, small), np.arange(1000))
    cols = bench.dump_columns(32, 2, True, capi.SUMMARY_DTYPE, grid=True)                 # cfg3's files
    row, head = 8 * sum(cols.values()), bench.NPY_HEADER_BYTES * len(cols)
    s = bench.dump_sample(10_000, cols)
    assert len(s) * row + head <= bench.DUMP_BYTES < (len(s) + 1) * row + head
    assert np.all(np.diff(s) > 0) and s[0] >= 0 and s[-1] < 10_000
    assert np.array_equal(s, bench.dump_sample(10_000, cols))         # the same barcodes every run
    budget = 10 * row + head
    assert np.array_equal(bench.dump_sample(10, cols, budget=budget), np.arange(10))
    assert len(bench.dump_sample(11, cols, budget=budget)) == 10


def test_write_dump_writes_float64_npy_files(tmp_path):
    import bench
    from demuxlet_amd import capi
    summ = np.zeros(3, dtype=capi.SUMMARY_DTYPE)
    summ["i_sing1"] = [2, 0, 1]
    summ["llk12"] = [-1.5, -2.5, -3.5]
    arrays = {"barcode_index": np.arange(3), "llks": np.ones((3, 4), dtype=np.float32), "llk0s": np.zeros(3), "l00": np.zeros((3, 2)),
              **bench.summary_columns(summ)}
    cols = bench.dump_columns(4, 2, True, capi.SUMMARY_DTYPE)
    rec = bench.write_dump(tmp_path / "d", arrays, cols)
    assert rec["barcodes"] == 3 and rec["bytes"] == _disk_bytes(tmp_path / "d") and rec["arrays"] == sorted(cols)
    for name in rec["arrays"]:
        a = np.load(tmp_path / "d" / f"{name}.npy")
        assert a.dtype == np.float64 and a.shape[0] == 3 and a.size == 3 * cols[name]
    assert np.array_equal(np.load(tmp_path / "d" / "summary_i_sing1.npy"), [2.0, 0.0, 1.0])
    # arrays that are not the planned files are refused before anything is written
    with pytest.raises(AssertionError):
        bench.write_dump(tmp_path / "e", {**arrays, "extra": np.zeros(3)}, cols)
    with pytest.raises(AssertionError):
        bench.write_dump(tmp_path / "f", {**arrays, "llks": np.zeros((3, 5))}, cols)
    assert not (tmp_path / "e").exists() and not (tmp_path / "f").exists()


def test_gathered_dump_of_the_default_sharded_workload_stays_within_the_budget(tmp_path):
    """The N > 1 default (cfg4: 100 000 barcodes, V = 64, A = 2) on 8 ranks: the records rank 0 gathers, here injected on the CPU in
    record_matrix's layout (padded to the largest count), through the dump.  The sample is as large as the budget allows and the files on
    disk stay within it."""
    import torch
    import bench
    from demuxlet_amd import engine
    cfg = bench.CONFIGS[4]
    V, A, world = cfg["V"], len(cfg["alphas"]), 8
    words = engine.capi.SUMMARY_DTYPE.itemsize // 8
    ncols = V + 1 + V + A + words
    counts = [bench.shard_range(cfg["B"], world, r)[1] - bench.shard_range(cfg["B"], world, r)[0] for r in range(world)]
    gathered = []
    for r in range(world):
        lo = bench.shard_range(cfg["B"], world, r)[0]
        rec = torch.zeros((max(counts), ncols), dtype=torch.float64)
        rec[:counts[r], 0] = torch.arange(lo, lo + counts[r], dtype=torch.float64)      # llks[:, 0] = the barcode's number
        gathered.append(rec)
    cx = types.SimpleNamespace(torch=torch, engine=engine)
    rec = bench.dump_gathered_outputs(cx, gathered, counts, cfg, tmp_path / "d")
    cols = bench.dump_columns(V, A, True, engine.capi.SUMMARY_DTYPE, sing=True)
    row, head = 8 * sum(cols.values()), bench.NPY_HEADER_BYTES * len(cols)
    assert rec["barcodes"] < cfg["B"] and (rec["barcodes"] + 1) * row + head > bench.DUMP_BYTES
    assert rec["bytes"] == _disk_bytes(tmp_path / "d") <= bench.DUMP_BYTES
    assert sorted(p.stem for p in (tmp_path / "d").glob("*.npy")) == sorted(cols)
    idx = np.load(tmp_path / "d" / "barcode_index.npy")
    assert len(idx) == rec["barcodes"] and np.array_equal(np.load(tmp_path / "d" / "llks.npy")[:, 0], idx)
