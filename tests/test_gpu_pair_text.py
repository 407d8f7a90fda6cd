"""GPU (-m gpu): the `.pair` rows of `--write-pair` (cmd_cram_demuxlet.cpp:772-797) formatted ON THE DEVICE (dmx_engine_format_pair, ABI 8;
csrc/dmx_format.hpp) are the host formatter's bytes.

* crafted grids: every magnitude a log-likelihood and a posterior can take (negative zero, subnormals, 1e-3 ... 8e12, the denormal range of exp, values that
  underflow for certain), nan / inf / |v| >= 2^43 (left to the host: flag 2) — field by field against Python's '%.5f' / '%.5g' (glibc printf);
* real problems: the text with its patches spliced in == the file dmx_write_doublet writes from the same grid;
* the job: dmx_demuxlet_run with write_pair, device formatting (default) vs the host formatter (DMX_PAIR_ON_HOST=1, fenced): four files byte for byte, one
  range and many, with barcodes whose rows stay on the host (duplicate samples -> near-tie flags);
* certified entries (K3b) that move a POSTPRB value across a rounding boundary (pair_craft.py): the device prints from the grid WITH them, as the host formatter
  does, and reports the three scalars it printed from;
* scalars that are not finite (a nan / inf in an entry that is never printed, or set directly): flag 2, the host prints the barcode;
* 225 ... 528 rows per barcode (one to three chunks of k_pair_write), any n_out / order / host_rows mask against the plain ascending call;
* the limits: the longest rows the device path takes (a 150 KiB LDS buffer), DMX_ERR_ARG one byte beyond, and a job beyond them falls back to the host formatter."""
import json
import math
import os

import numpy as np
import pytest

import pair_craft as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    from demuxlet_amd import build, capi, engine
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return engine


def small_engine(eng, V, alphas, B, S=60, seed=3, dup=False):
    from demuxlet_amd import synth
    rng = np.random.default_rng(seed)
    raw = synth.make_raw_genotypes(rng, S, V)
    if dup and V >= 4:
        raw.alleles[:, 1] = raw.alleles[:, 0]
    g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    sp = synth.make_pileup(rng, raw.alleles, B, 0.5, 1.5, doublet_rate=0.3)
    pl = eng.HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads, sp.rd_totl, sp.rd_pass, sp.rd_uniq)
    e = eng.Engine(V, alphas, 0.5)
    e.set_genotypes(g); e.set_pileup(pl); e.run(); e.sync()
    return e, g, sp, pl


def rows_of(V, alphas):
    out = []
    for j in range(V):
        out.append((j, j, 0))
        for k in range(V):
            for a in range(1, len(alphas)):
                if j == k or (j > k and alphas[a] == 0.5):
                    continue
                out.append((j, k, a))
    return out


def splice(text, patches, scal, V, A, prior):
    """The text with the fields the device left to the host's libm filled in (what dmx_demuxlet_run's writer does): from the three scalars the call reports
    per OUTPUT barcode (format_pair(..., scalars=True)) — K3's record, or the certified grid's."""
    out, pos = [], 0
    for off, v, oc, singlet in patches:
        out.append(text[pos:off]); pos = off
        sm = scal[oc]
        tot = float(sm["sum_single"]) + float(sm["sum_double"])
        x = v - float(sm["max_llk"])
        e = math.exp(x)
        p = e * (1. - prior) / V / tot if singlet else e * prior / V / (V - 1) / (A - 1) / tot
        out.append(("%.5g" % p).encode())
    out.append(text[pos:])
    return b"".join(out)


def poke(eng, e, B, V, A, vals, set_summ):
    """Write vals [B][V][V][A] into the staged engine's llksAB and let set_summ(records) edit its K3 records, through device_view.  Returns the records."""
    import torch
    from demuxlet_amd import synth_torch as st
    dev = torch.device("cuda", 0)
    view = e.device_view()
    grid = st.tensor_from_ptr(view.llksAB, (B, V, V, A), torch.float64, dev)
    words = eng.capi.SUMMARY_DTYPE.itemsize // 8
    summ_t = st.tensor_from_ptr(view.summary, (B, words), torch.float64, dev)
    grid.copy_(torch.from_numpy(np.ascontiguousarray(vals)).to(dev))
    summ = np.ascontiguousarray(summ_t.cpu().numpy()).view(eng.capi.SUMMARY_DTYPE).reshape(-1).copy()
    set_summ(summ)
    summ_t.copy_(torch.from_numpy(summ.view(np.float64).reshape(B, words)).to(dev))
    torch.cuda.synchronize()
    return summ


def crafted_values(rng, B, V, A):
    """Every magnitude a log-likelihood and a posterior can take (see the module docstring); `special` barcodes hold an unprintable LLK."""
    vals = np.empty((B, V, V, A))
    kind = rng.integers(0, 8, size=vals.shape)
    vals[:] = -rng.uniform(0, 760, size=vals.shape)                                   # posterior from 1 down through the denormal range to 0
    vals[kind == 1] = -np.exp(rng.uniform(np.log(1e-3), np.log(8e12), size=(kind == 1).sum()))
    vals[kind == 2] = np.exp(rng.uniform(np.log(1e-320), np.log(1e-3), size=(kind == 2).sum()))   # subnormal ... tiny positive
    vals[kind == 3] = -rng.uniform(0, 50, size=(kind == 3).sum())                       # posteriors that print in fixed notation
    vals[kind == 4] = np.round(-rng.uniform(0, 1e5, size=(kind == 4).sum()), 5)         # decimal-looking values (ties of the 6th digit)
    vals[kind == 5] = -rng.uniform(800, 2e5, size=(kind == 5).sum())                    # posteriors that underflow for certain: "0" without exp()
    vals.reshape(-1)[:8] = [-0.0, 0.0, -5e-324, 2.5e-6, -2.5e-6, 1.5e-5, -99999.999995, -123456.785]
    special = np.zeros(B, dtype=bool)
    for c, v in ((5, np.nan), (6, np.inf), (7, -np.inf), (8, -9e12), (9, 2.0 ** 43)):
        vals[c, 3, 4, 1] = v; special[c] = True
    return vals, special


def free_summary(rng, B):
    def set_summ(summ):
        summ["max_llk"] = 0.0
        summ["sum_single"] = rng.uniform(0.2, 0.9, size=B); summ["sum_double"] = rng.uniform(0.0, 0.5, size=B)
        summ["max_llk"][B // 30:B // 15] = rng.uniform(-3, 3, size=B // 15 - B // 30)
    return set_summ


def crafted_field_by_field(eng, V, alphas, B):
    """Returns (fields printed on the device, fields left to the host, the largest number of different 256-row chunks one barcode has patches in)."""
    A = len(alphas)
    e, g, sp, pl = small_engine(eng, V, alphas, B)
    rng = np.random.default_rng(11)
    vals, special = crafted_values(rng, B, V, A)
    summ = poke(eng, e, B, V, A, vals, free_summary(rng, B))
    cells = np.arange(B, dtype=np.int32)[::-1].copy()                                   # any output order
    bcs = [f"BC{c:05d}-1" for c in cells]
    sms = [f"S{j}x" * (1 + j % 3) for j in range(V)]
    text, off, flag, patches, ms = e.format_pair(cells, bcs, sms)
    assert [int(f) for f in flag] == [2 if special[c] else 0 for c in cells]
    assert all(off[i + 1] == off[i] for i in range(B) if flag[i])
    pat = {}
    for o, v, oc, sg in patches:
        pat[o] = (v, oc, sg)
    rows = rows_of(V, alphas)
    n_fields = n_patched = max_chunks = 0
    for i, c in enumerate(cells):
        if flag[i]:
            continue
        chunks = set()
        seg = text[off[i]:off[i + 1]]
        lines = seg.split(b"\n")
        assert lines[-1] == b"" and len(lines) == len(rows) + 1
        pos = int(off[i])
        tot = float(summ["sum_single"][c]) + float(summ["sum_double"][c])
        for r, ((j, k, a), ln) in enumerate(zip(rows, lines)):
            f = ln.split(b"\t")
            v = vals[c, j, 0 if a == 0 else k, a]
            assert f[0] == bcs[i].encode() and f[1] == sms[j].encode() and f[2] == sms[k].encode() and f[3] == (b"%.3f" % alphas[a])
            assert f[4] == ("%.5f" % v).encode(), (c, j, k, a, v, f[4])
            post_at = pos + len(ln) - len(f[5])
            x = v - float(summ["max_llk"][c])
            if post_at in pat and f[5] == b"":
                assert pat[post_at] == (v, i, 1 if a == 0 else 0)
                n_patched += 1
                chunks.add(r // 256)
            else:
                assert post_at not in pat
                ex = math.exp(x)
                p = ex * (1. - 0.5) / V / tot if a == 0 else ex * 0.5 / V / (V - 1) / (A - 1) / tot
                assert f[5] == ("%.5g" % p).encode(), (c, j, k, a, v, p, f[5])
                n_fields += 1
            pos += len(ln) + 1
        assert pos == off[i + 1]
        max_chunks = max(max_chunks, len(chunks))
    assert len(pat) == n_patched
    print(f"{n_fields} POSTPRB fields printed on the device, {n_patched} left to the host; {ms:.2f} ms")
    e.close()
    return n_fields, n_patched, max_chunks


def test_crafted_values_field_by_field(eng):
    n_fields, n_patched, _ = crafted_field_by_field(eng, 8, (0.0, 0.5), 3000)
    assert n_fields > 50_000 and 0 < n_patched < n_fields // 4


# rows per barcode: 225 (under one 256-row chunk of k_pair_write), 256 (exactly one), 289 (one and a tail), 376 (A = 3), 528 (three chunks)
@pytest.mark.parametrize("V,alphas,B", [(15, (0.0, 0.25), 300), (16, (0.0, 0.25), 250), (17, (0.0, 0.25), 220), (16, (0.0, 0.25, 0.5), 160), (32, (0.0, 0.5), 120)])
def test_crafted_values_across_chunks(eng, V, alphas, B):
    n_rows = len(rows_of(V, alphas))
    assert n_rows == {15: 225, 17: 289, 32: 528}.get(V, 256 if len(alphas) == 2 else 376)
    n_fields, n_patched, max_chunks = crafted_field_by_field(eng, V, alphas, B)
    assert n_fields > 50_000 * (B * n_rows) // (3000 * 36) and 0 < n_patched < n_fields // 4      # the bound of the 36-row test, per field
    assert max_chunks >= min(2, (n_rows + 255) // 256)          # patch indices carried across a chunk boundary (pbase += ptotal)


@pytest.mark.parametrize("V,alphas,dup", [(4, (0.0, 0.5), False), (12, (0.0, 0.25, 0.5), False), (7, (0.1, 0.5, 0.9), False), (33, (0.0, 0.5), True)])
def test_device_text_is_the_host_formatters_file(eng, tmp_path, V, alphas, dup):
    B = 150
    e, g, sp, pl = small_engine(eng, V, alphas, B, S=40 if V < 30 else 25, seed=V, dup=dup)
    grid, l00, summ = e.get_doublet()
    A = len(alphas)
    bcs = [f"BC{(i * 7919) % 1000:04d}-1" for i in range(B)]
    sms = [f"SM{j:02d}" for j in range(V)]
    fa = eng.FinalArgs(bcs, sms, alphas, 0.5, sp.rd_totl, sp.rd_pass, sp.rd_uniq, pl.n_snp_per_cell, write_pair=True)
    eng.write_doublet(fa, grid, l00, str(tmp_path / "h"))                                # host formatter, no arbiter: the device grid as it is
    order = sorted(range(B), key=lambda i: bcs[i].encode())
    cells = np.array([i for i in order if pl.n_snp_per_cell[i] > 0], dtype=np.int32)
    # what the host formatter prints for the certified entries of an alpha = 0.5 best doublet (no near-tie flag): the certificate's values
    ovr = []
    for c in cells:
        sm = summ[c]
        if (sm["flags"] & eng.capi.DMX_CELL_ORDER_RESOLVABLE):
            one = summ[c:c + 1].copy(); eng.resolve_tie_order(one); sm = one[0]
        if (sm["flags"] & eng.capi.DMX_CELL_ORDER_CERTIFIED) and not (sm["flags"] & 3):
            ovr.append((min(sm["j_best"], sm["k_best"]), max(sm["j_best"], sm["k_best"]), sm["n_best"], 0, sm["llk_ab"], sm["llk_ba"]))
        else:
            ovr.append(None)
    text, off, flag, patches, ms, scal = e.format_pair(cells, [bcs[c] for c in cells], sms, ovr=ovr, scalars=True)
    assert not flag.any()
    # the host formatter takes maxLLK and the two sums from the (certified) grid with the host libm; the device text uses the scalars it reports (K3's
    # record, or the certified grid's) — equal to the last digit printed
    got = b"BARCODE\tSM1.ID\tSM2.ID\tLLK12\tPOSTPRB\n" + splice(text, patches, scal, V, A, 0.5)
    want = (tmp_path / "h.pair").read_bytes()
    assert got == want
    e.close()


@pytest.mark.parametrize("V,field,mode,rb", [(6, "GT", "strict", None), (6, "GT", "strict", "20000"), (16, "GP", "fast", "60000"), (5, "GT", "strict", "9000")])
def test_job_with_write_pair_device_vs_host_formatter(eng, tmp_path, monkeypatch, V, field, mode, rb):
    from demuxlet_amd import synth, capi
    rng = np.random.default_rng(900 + V)
    S, B = 300, 400
    raw = synth.make_raw_genotypes(rng, S, V)
    if V == 5:                                      # duplicate samples: near-tie flags -> barcodes whose rows stay on the host formatter
        raw.alleles[:, 1] = raw.alleles[:, 0]; raw.alleles[:, 3] = raw.alleles[:, 2]
    if field == "GT":
        g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    else:
        g = np.stack([eng.geno_from_gp(x, 0.01) for x in synth.raw_gp_from_alleles(rng, raw.alleles)])
    sp = synth.make_pileup(rng, raw.alleles, B, 0.05 if V == 5 else 0.3, 1.5, doublet_rate=0.4)
    pl = eng.HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads, sp.rd_totl, sp.rd_pass, sp.rd_uniq)
    bcs = [f"BC{(i * 7919) % 100003:06d}-1" for i in range(B)]
    sms = [f"S{j:02d}" for j in range(V)]
    md = capi.DMX_MODE_FAST if mode == "fast" else capi.DMX_MODE_STRICT
    monkeypatch.setenv("DMX_EXPERIMENTS", "1")
    if rb: monkeypatch.setenv("DMX_RANGE_BYTES", rb)
    else: monkeypatch.delenv("DMX_RANGE_BYTES", raising=False)
    monkeypatch.delenv("DMX_PAIR_ON_HOST", raising=False)
    td = eng.demuxlet_run(pl, g, sms, (0.0, 0.5), str(tmp_path / "d"), write_pair=True, barcodes=bcs, mode=md, timing=True)
    monkeypatch.setenv("DMX_PAIR_ON_HOST", "1")
    th = eng.demuxlet_run(pl, g, sms, (0.0, 0.5), str(tmp_path / "h"), write_pair=True, barcodes=bcs, mode=md, timing=True)
    assert td["n_ranges"] == th["n_ranges"] and (rb is None or td["n_ranges"] > 2)
    for suf in ("single", "sing2", "best", "pair"):
        assert (tmp_path / f"d.{suf}").read_bytes() == (tmp_path / f"h.{suf}").read_bytes(), suf
    n_rows = sum(1 for _ in open(tmp_path / "d.pair")) - 1
    covered = int((pl.n_snp_per_cell > 0).sum())
    assert n_rows == covered * (V + V * (V - 1) // 2)


def set_records(scalars):
    """Records as K3 leaves them for the given (max_llk, sum_single, sum_double) per cell."""
    def set_summ(summ):
        for c, (mx, ss, sd) in enumerate(scalars):
            summ["max_llk"][c] = mx; summ["sum_single"][c] = ss; summ["sum_double"][c] = sd
    return set_summ


def host_pair_rows(eng, tmp_path, grids, bcs, sms, alphas, name="h"):
    """The host formatter's `.pair` rows of every barcode, keyed by cell: dmx_write_doublet from the given grids (no records: what it prints is the grid's)."""
    B, V, A = grids.shape[0], grids.shape[1], len(alphas)
    ones = np.ones(B, dtype=np.int32)
    fa = eng.FinalArgs(bcs, sms, alphas, 0.5, ones, ones, ones, ones, write_pair=True)
    eng.write_doublet(fa, grids, np.zeros((B, A)), str(tmp_path / name))
    data = (tmp_path / f"{name}.pair").read_bytes()
    head = b"BARCODE\tSM1.ID\tSM2.ID\tLLK12\tPOSTPRB\n"
    assert data.startswith(head)
    lines = data[len(head):].split(b"\n")
    assert lines[-1] == b""
    n = len(rows_of(V, alphas))
    order = sorted(range(B), key=lambda i: bcs[i].encode())
    assert len(lines) - 1 == B * n
    return data, {c: b"".join(ln + b"\n" for ln in lines[q * n:(q + 1) * n]) for q, c in enumerate(order)}


@pytest.mark.parametrize("V,alphas", [(4, (0.0, 0.5)), (7, (0.0, 0.25, 0.5)), (4, (0.0, 0.25, 0.5)), (7, (0.0, 0.5))])
def test_certified_entries_move_a_digit_across_a_rounding_boundary(eng, tmp_path, V, alphas):
    """Barcodes whose K3b certificate lies 5e-12 / 5e-11 off the grid's entries, with one row tuned so that the digit depends on which of the two the sums were
    taken from (pair_craft.straddle_case; test_pair_craft_cpu.py checks the construction).  The records hold K3's scalars of the UNCERTIFIED grid; the text has
    to be the host formatter's, which prints from the grid with the certified entries.  No other row of these barcodes is within 1e-9 of a boundary, so the
    only field that may be left to the host is the probe's: handing the barcodes or their rows to the host does not pass.
    Cells 0-15: override off the grid's bits; 16-31: the same grids without an override; 32-47: an override equal to the grid's bits; 48-63: the
    certified values in the grid itself, no override."""
    A = len(alphas)
    cases = pc.straddle_cases(V, alphas, reps=2, seed=1)
    n = len(cases)
    assert n == 16
    B = 4 * n
    e, g, sp, pl = small_engine(eng, V, alphas, B)
    vals = np.stack([c.grid for c in cases] * 3 + [pc.substituted(c.grid, c.ovr) for c in cases])
    want_grid = vals.copy()
    ovr_of = [None] * B
    for q, c in enumerate(cases):
        a, b, h, v_ab, v_ba = c.ovr
        want_grid[q] = pc.substituted(c.grid, c.ovr)
        ovr_of[q] = (a, b, h, 0, v_ab, v_ba)
        ovr_of[2 * n + q] = (a, b, h, 0, float(c.grid[a, b, h]), float(c.grid[b, a, h]))
    k3 = [pc.k3_scalars(vals[c], alphas) for c in range(B)]                             # of the grid as it lies in memory: what K3 leaves
    poke(eng, e, B, V, A, vals, set_records(k3))
    bcs = [f"BC{(c * 37) % B:03d}-1" for c in range(B)]
    sms = [f"SM{j:02d}" for j in range(V)]
    data, want = host_pair_rows(eng, tmp_path, want_grid, bcs, sms, alphas)
    cells = np.array(sorted(range(B), key=lambda c: bcs[c].encode()), dtype=np.int32)
    text, off, flag, patches, ms, scal = e.format_pair(cells, [bcs[c] for c in cells], sms, ovr=[ovr_of[c] for c in cells], scalars=True)
    assert not flag.any()
    rows = rows_of(V, alphas)
    assert b"BARCODE\tSM1.ID\tSM2.ID\tLLK12\tPOSTPRB\n" + splice(text, patches, scal, V, A, 0.5) == data
    # the scalars the call reports: the certified grid's where the override changes the grid (the maximum exactly; the sums to the rounding of 2 V^2 A
    # terms, device exp and tree order against libm and serial order: far inside the 4e-13 margin), the record's bits everywhere else
    tol = (2 * V * V * A + 4) * 2.0 ** -52
    for i, c in enumerate(cells):
        got3 = (float(scal["max_llk"][i]), float(scal["sum_single"][i]), float(scal["sum_double"][i]))
        if c < n:
            w3 = pc.k3_scalars(want_grid[c], alphas)
            assert got3[0] == w3[0] and abs(got3[1] - w3[1]) <= tol * w3[1] and abs(got3[2] - w3[2]) <= tol * w3[2], (c, got3, w3)
            assert got3 != k3[c]
        else:
            assert got3 == k3[c], (c, got3, k3[c])
    # no field but the probe's may be left to the host
    n_probe_patches = 0
    for o, v, oc, sg in patches:
        c = int(cells[oc])
        seg = text[off[oc]:o]
        r = seg.count(b"\n")
        assert rows[r] == cases[c % n].probe, (c, rows[r], cases[c % n].probe)
        n_probe_patches += 1
    print(f"{n_probe_patches} probe fields left to the host of {B} (none is within the margin by construction); {ms:.2f} ms")
    # and the probe rows print the certified digits where the override differs from the grid, the grid's own digits elsewhere
    for c in range(n):
        case = cases[c]
        r = rows.index(case.probe)
        v = float(case.grid[pc.entry_of(case.probe)])
        f_cert = want[c].split(b"\n")[r].split(b"\t")[5]
        f_plain = want[n + c].split(b"\n")[r].split(b"\t")[5]
        assert f_cert == ("%.5g" % pc.host_post(v, pc.k3_scalars(want_grid[c], alphas), V, A, case.probe[2] == 0)).encode()
        assert f_plain == ("%.5g" % pc.host_post(v, k3[c], V, A, case.probe[2] == 0)).encode() and f_plain != f_cert
        assert want[2 * n + c].split(b"\n")[r].split(b"\t")[5] == f_plain and want[3 * n + c].split(b"\n")[r].split(b"\t")[5] == f_cert
    e.close()


@pytest.mark.parametrize("V,alphas", [(4, (0.0, 0.5)), (5, (0.0, 0.25, 0.5))])
def test_scalars_that_are_not_finite_leave_the_barcode_to_the_host(eng, tmp_path, V, alphas):
    """maxLLK is the maximum of the WHOLE grid and sumDouble covers the j > k entries at alpha 0.5 too: a nan / inf in an entry that is never printed makes
    the sum nan or the maximum infinite although every printed LLK is fine.  The host formatter prints `nan` posteriors for such a barcode; the device's
    "0" shortcuts (x < -800, p == 0) hold for finite scalars only, so it hands the barcode over: flag 2, an empty range.  Neighbours are untouched."""
    A = len(alphas)
    B = 64
    half = max(a for a in range(1, A) if alphas[a] == 0.5)
    e, g, sp, pl = small_engine(eng, V, alphas, B)
    rng = np.random.default_rng(23)
    vals = -50.0 - rng.uniform(0.0, 600.0, size=(B, V, V, A))
    vals[:, 0, 1, half] = -50.0                                                          # a clear best doublet
    nan, inf = math.nan, math.inf
    in_grid = {4: ((2, 1, half), nan),               # j > k at alpha 0.5: never printed, summed -> tot is nan
               5: ((3, 0, half), nan),
               9: ((1, 1, 1), inf),                  # the diagonal: never printed, never summed, but the maximum -> max_llk = inf, tot = 0
               10: ((2, 2, A - 1), inf),
               14: ((1, 2, 0), inf),                 # n = 0, k > 0: likewise
               15: ((0, V - 1, 0), inf)}
    for c, (idx, v) in in_grid.items():
        vals[(c,) + idx] = v
    k3 = [pc.k3_scalars(vals[c], alphas) for c in range(B)]
    for c in (4, 5):
        assert math.isnan(k3[c][1] + k3[c][2]) and math.isfinite(k3[c][0])
    for c in (9, 10, 14, 15):
        assert k3[c][0] == inf and k3[c][1] + k3[c][2] == 0.0
    direct = {20: (None, 0.0, 0.0), 21: (None, 0.25, -0.5), 22: (None, -1e-300, 0.0), 23: (None, inf, 0.1), 24: (None, 0.1, inf), 25: (None, nan, 0.1),
              26: (None, 0.1, nan), 27: (None, inf, -inf),
              30: (nan, None, None), 31: (inf, None, None), 32: (-inf, None, None),
              63: (nan, nan, nan), 0: (inf, 0.0, 0.0)}                                   # the first and the last output barcode too
    for c, (mx, ss, sd) in direct.items():
        k3[c] = (k3[c][0] if mx is None else mx, k3[c][1] if ss is None else ss, k3[c][2] if sd is None else sd)
    bad = set(in_grid) | set(direct)
    poke(eng, e, B, V, A, vals, set_records(k3))
    bcs = [f"BC{c:03d}-1" for c in range(B)]
    sms = [f"SM{j:02d}" for j in range(V)]
    data, want = host_pair_rows(eng, tmp_path, vals, bcs, sms, alphas)
    for c in in_grid:                                                                    # what the host makes of them: nan posteriors
        assert all(ln.split(b"\t")[5] in (b"nan", b"-nan") for ln in want[c].split(b"\n")[:-1]), want[c][:200]
    cells = np.arange(B, dtype=np.int32)
    text, off, flag, patches, ms, scal = e.format_pair(cells, bcs, sms, scalars=True)
    assert [int(f) for f in flag] == [2 if c in bad else 0 for c in range(B)]
    assert all(off[c + 1] == off[c] for c in bad) and off[B] == len(text)
    assert all(cells[oc] not in bad for _, _, oc, _ in patches)
    # every other barcode: its bytes, patches filled in, are the host formatter's
    full = splice(text, patches, scal, V, A, 0.5)
    by_cell = {c: [] for c in range(B)}
    for o, v, oc, sg in patches:
        by_cell[int(cells[oc])].append((o - int(off[oc]), v, 0, sg))
    for c in range(B):
        if c in bad:
            continue
        seg = splice(text[off[c]:off[c + 1]], by_cell[c], [scal[c]], V, A, 0.5)
        assert seg == want[c], c
    assert full == b"".join(want[c] for c in range(B) if c not in bad)
    e.close()


def per_barcode(text, off, flag, patches, n):
    """[(flag, segment bytes, [(offset within the segment, value, singlet)])] per output barcode, with the structural checks every call has to pass."""
    assert off[0] == 0 and off[n] == len(text) and all(off[i] <= off[i + 1] for i in range(n))
    assert all(patches[i][0] < patches[i + 1][0] for i in range(len(patches) - 1))
    out = [(int(flag[i]), text[off[i]:off[i + 1]], []) for i in range(n)]
    for o, v, oc, sg in patches:
        assert 0 <= oc < n and off[oc] <= o < off[oc + 1] and flag[oc] == 0
        out[oc][2].append((o - int(off[oc]), v, sg))
    for i in range(n):
        assert flag[i] == 0 or (off[i] == off[i + 1] and not out[i][2])
    return out


def compare_with_plain_call(e, base, cells, bcs, sms, host_rows=None):
    n = len(cells)
    text, off, flag, patches, ms = e.format_pair(cells, [bcs[c] for c in cells], sms, host_rows=host_rows)
    got = per_barcode(text, off, flag, patches, n)
    for i, c in enumerate(cells):
        if host_rows is not None and host_rows[i]:
            assert got[i][0] == 1 and off[i] == off[i + 1], (i, c)
        else:
            assert got[i] == base[c], (i, c)
    return got


def crafted_engine_and_plain_call(eng, V, alphas, B, flagged, seed):
    A = len(alphas)
    e, g, sp, pl = small_engine(eng, V, alphas, B)
    rng = np.random.default_rng(seed)
    vals, special = crafted_values(rng, B, V, A)
    vals[special, 3 % V, 4 % V, 1] = -1.0
    for c in flagged:
        vals[c, 1, 2, 1] = np.nan
    poke(eng, e, B, V, A, vals, free_summary(rng, B))
    bcs = [f"BC{c:05d}-1" for c in range(B)]
    sms = [f"S{j}x" * (1 + j % 3) for j in range(V)]
    cells = np.arange(B, dtype=np.int32)
    text, off, flag, patches, ms = e.format_pair(cells, bcs, sms)
    base = per_barcode(text, off, flag, patches, B)
    assert [b[0] for b in base] == [2 if c in flagged else 0 for c in range(B)]
    assert sum(len(b[2]) for b in base) > B                                            # dense in patches
    return e, base, bcs, sms


def test_output_orders_and_host_rows_masks_against_the_plain_call(eng):
    """289 rows per barcode (a chunk and a tail).  Whatever the order of the output barcodes and whichever of them the caller keeps (host_rows), every other
    barcode's bytes and patches — offsets relative to its segment — are those of the plain ascending call; kept and flag-2 barcodes have empty ranges at
    their place.  Flag-2 barcodes sit next to the kept ones."""
    V, alphas, B = 17, (0.0, 0.25), 48
    flagged = {1, 9, 12, B - 2}
    e, base, bcs, sms = crafted_engine_and_plain_call(eng, V, alphas, B, flagged, seed=5)
    assert any(len({b[1][:o].count(b"\n") // 256 for o, _, _ in b[2]}) > 1 for b in base)     # patches on either side of the chunk boundary
    text, off, flag, patches, ms = e.format_pair(np.zeros(0, dtype=np.int32), [], sms)
    assert text == b"" and list(off) == [0] and len(flag) == 0 and patches == []
    rng = np.random.default_rng(6)
    asc = np.arange(B, dtype=np.int32)
    for cells in (asc[:1], asc[:2], asc[1:3], asc[::-1].copy(), rng.permutation(B).astype(np.int32), asc[B - 3:]):
        compare_with_plain_call(e, base, cells, bcs, sms)
    masks = {"first": [0], "last": [B - 1], "adjacent": [10, 11], "alternating": list(range(0, B, 2)), "all": list(range(B)),
             "around flagged": [0, 2, 8, 10, 11, 13, B - 3, B - 1]}
    for name, idx in masks.items():
        hr = np.zeros(B, dtype=np.uint8); hr[idx] = 1
        got = compare_with_plain_call(e, base, asc, bcs, sms, host_rows=hr)
        assert [x[0] for x in got] == [1 if hr[c] else (2 if c in flagged else 0) for c in range(B)], name
    hr = np.zeros(B, dtype=np.uint8); hr[::3] = 1                                      # a mask with an order of its own
    perm = rng.permutation(B).astype(np.int32)
    compare_with_plain_call(e, base, perm, bcs, sms, host_rows=hr[perm])
    e.close()


def test_output_counts_around_the_scan_widths(eng):
    """k_pair_scan gives each of its 1024 threads ceil(n_out / 1024) barcodes: 1023, 1024, 1025 and 2049 barcodes sit on either side of one and of two per
    thread.  10 rows per barcode (V = 4)."""
    V, alphas, B = 4, (0.0, 0.5), 2100
    flagged = {0, 1022, 1023, 1024, 2047, 2048}
    e, g, sp, pl = small_engine(eng, V, alphas, B)
    A = len(alphas)
    rng = np.random.default_rng(17)
    vals = -rng.uniform(0, 760, size=(B, V, V, A))                                      # through the denormal range: patches
    for c in flagged:
        vals[c, 1, 2, 1] = np.inf
    poke(eng, e, B, V, A, vals, free_summary(rng, B))
    bcs = [f"BC{c:05d}-1" for c in range(B)]
    sms = [f"S{j}" for j in range(V)]
    asc = np.arange(B, dtype=np.int32)
    text, off, flag, patches, ms = e.format_pair(asc, bcs, sms)
    base = per_barcode(text, off, flag, patches, B)
    assert [b[0] for b in base] == [2 if c in flagged else 0 for c in range(B)]
    assert len(patches) > B // 2                       # about one row in ten lies in the denormal range of exp: about one patch per barcode
    for n_out in (0, 1, 2, 1023, 1024, 1025, 2049):
        compare_with_plain_call(e, base, asc[:n_out], bcs, sms)
    compare_with_plain_call(e, base, asc[::-1][:2049].copy(), bcs, sms)
    perm = rng.permutation(B).astype(np.int32)[:2049]
    hr = (rng.integers(0, 3, size=2049) == 0).astype(np.uint8)
    compare_with_plain_call(e, base, perm, bcs, sms)
    compare_with_plain_call(e, base, perm, bcs, sms, host_rows=hr)
    e.close()


def longest_ids(alphas, bc_len):
    """The longest sample id the device path takes with barcodes of bc_len bytes, from the limit dmx.h states: 256 rows of up to
    bc + 1 + sm + 1 + sm + len("\\t%.3lf\\t") + 20 (LLK) + 1 + 12 (POSTPRB) + 1 bytes in 150 KiB."""
    al = max(len("\t%.3f\t" % a) for a in alphas)
    max_row = lambda s: bc_len + 1 + 2 * s + 1 + al + 20 + 1 + 12 + 1
    s = 1
    while 256 * max_row(s + 1) <= 150 * 1024:
        s += 1
    assert 256 * max_row(s) <= 150 * 1024 < 256 * max_row(s + 1)
    return s, 256 * max_row(s)


def certified_overrides(eng, summ, cells):
    """What the host formatter prints for the certified entries of an alpha = 0.5 best doublet (no near-tie flag): the certificate's values."""
    ovr = []
    for c in cells:
        sm = summ[c]
        if (sm["flags"] & eng.capi.DMX_CELL_ORDER_RESOLVABLE):
            one = summ[c:c + 1].copy(); eng.resolve_tie_order(one); sm = one[0]
        if (sm["flags"] & eng.capi.DMX_CELL_ORDER_CERTIFIED) and not (sm["flags"] & 3):
            ovr.append((min(sm["j_best"], sm["k_best"]), max(sm["j_best"], sm["k_best"]), sm["n_best"], 0, sm["llk_ab"], sm["llk_ba"]))
        else:
            ovr.append(None)
    return ovr


def test_longest_rows_the_device_path_takes_and_one_byte_more(eng, tmp_path):
    """Sample ids at the limit: k_pair_write's LDS buffer is then as large as the device path allows (150 KiB less a few bytes; the other tests stay under
    10 KB) and the bytes are still the host formatter's.  One byte more per id is DMX_ERR_ARG, as dmx.h says."""
    V, alphas, B = 5, (0.0, 0.5), 40
    A = len(alphas)
    e, g, sp, pl = small_engine(eng, V, alphas, B, seed=8)
    grid, l00, summ = e.get_doublet()
    bcs = [f"BC{(i * 7919) % 1000000:06d}-1" for i in range(B)]
    assert all(len(b) == 10 for b in bcs)
    s_ok, lds = longest_ids(alphas, 10)
    assert lds > 149 * 1024
    order = sorted(range(B), key=lambda i: bcs[i].encode())
    cells = np.array([i for i in order if pl.n_snp_per_cell[i] > 0], dtype=np.int32)
    ovr = certified_overrides(eng, summ, cells)
    sms = [(f"S{j}-" + "x" * s_ok)[:s_ok] for j in range(V)]
    fa = eng.FinalArgs(bcs, sms, alphas, 0.5, sp.rd_totl, sp.rd_pass, sp.rd_uniq, pl.n_snp_per_cell, write_pair=True)
    eng.write_doublet(fa, grid, l00, str(tmp_path / "h"))
    text, off, flag, patches, ms, scal = e.format_pair(cells, [bcs[c] for c in cells], sms, ovr=ovr, scalars=True)
    assert not flag.any() and len(cells) > B // 2
    got = b"BARCODE\tSM1.ID\tSM2.ID\tLLK12\tPOSTPRB\n" + splice(text, patches, scal, V, A, 0.5)
    assert got == (tmp_path / "h.pair").read_bytes()
    longer = [(f"S{j}-" + "x" * (s_ok + 1))[:s_ok + 1] for j in range(V)]
    with pytest.raises(eng.capi.DmxError) as ei:
        e.format_pair(cells, [bcs[c] for c in cells], longer, ovr=ovr)
    assert ei.value.code == eng.capi.DMX_ERR_ARG
    extra = (150 * 1024 - lds) // 256 + 1
    with pytest.raises(eng.capi.DmxError) as ei:                                        # one long barcode does it too
        e.format_pair(cells[:2], [bcs[cells[0]], bcs[cells[1]] + "y" * extra], sms)
    assert ei.value.code == eng.capi.DMX_ERR_ARG
    e.close()


@pytest.mark.parametrize("beyond", [0, 1])
def test_job_at_and_beyond_the_device_paths_limits(eng, tmp_path, monkeypatch, capfd, beyond):
    """dmx_demuxlet_run with write_pair and sample ids at the limit of the device path (formatted on the device) and one byte beyond (the job falls back to
    the host formatter instead of failing): the four files equal those of the host formatter (DMX_PAIR_ON_HOST=1) byte for byte."""
    from demuxlet_amd import synth, capi
    V, S, B = 3, 200, 100
    rng = np.random.default_rng(77)
    raw = synth.make_raw_genotypes(rng, S, V)
    g = np.stack([eng.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    sp = synth.make_pileup(rng, raw.alleles, B, 0.3, 1.5, doublet_rate=0.4)
    pl = eng.HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, sp.pair_nrd, sp.reads, sp.rd_totl, sp.rd_pass, sp.rd_uniq)
    bcs = [f"BC{(i * 7919) % 100003:06d}-1" for i in range(B)]
    assert all(len(b) == 10 for b in bcs) and len(set(bcs)) == B
    alphas = (0.0, 0.5)
    s_ok, _ = longest_ids(alphas, 10)
    n = s_ok + beyond
    sms = [(f"S{j}-" + "y" * n)[:n] for j in range(V)]
    monkeypatch.setenv("DMX_EXPERIMENTS", "1")
    monkeypatch.setenv("DMX_E2E_TIMING", "1")
    monkeypatch.delenv("DMX_RANGE_BYTES", raising=False)

    def run(prefix):
        capfd.readouterr()
        eng.demuxlet_run(pl, g, sms, alphas, str(tmp_path / prefix), write_pair=True, barcodes=bcs, mode=capi.DMX_MODE_STRICT, timing=True)
        err = capfd.readouterr().err
        recs = [json.loads(ln)["dmx_demuxlet_run"] for ln in err.splitlines() if ln.startswith('{"dmx_demuxlet_run"')]
        assert len(recs) == 1, err
        return recs[0]

    monkeypatch.delenv("DMX_PAIR_ON_HOST", raising=False)
    td = run("d")
    monkeypatch.setenv("DMX_PAIR_ON_HOST", "1")
    th = run("h")
    assert td["pair_on_device"] == (0 if beyond else 1) and th["pair_on_device"] == 0
    for suf in ("single", "sing2", "best", "pair"):
        assert (tmp_path / f"d.{suf}").read_bytes() == (tmp_path / f"h.{suf}").read_bytes(), suf
    covered = int((pl.n_snp_per_cell > 0).sum())
    assert sum(1 for _ in open(tmp_path / "d.pair")) - 1 == covered * (V + V * (V - 1) // 2) and covered > B // 2
