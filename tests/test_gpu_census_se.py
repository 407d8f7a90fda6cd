"""GPU (-m gpu): census uncertainty (Engine.census_fisher, gap_on_support, census.py's --se / --presence).

The pass is checked against the float64 numpy restatement of tests/census_se_ref.py.  The restatement forms every term of H with the
device's operations on the device's operands: A_i, P_r, the two quotients and the five per-pair sums (reads in stored order) carry the
same bits, and so do the nine roundings of a term.  It then adds the terms in extended precision (one rounding).  The device adds a
chunk's terms serially (one rounding per pair, each relative to a partial sum that is at most the total: every term is non-negative),
folds the chunks into eight accumulators (one rounding per chunk) and adds those (three).  With P the group's counted pairs,
  |d H_vu| <= 2^-53 (P + chunks + 4) H_vu <= 2^-52 (P + 16) H_vu,
tighter than 2^-52 (2 (T + V + 8) + 8) H_vu, T = reads + 2 pairs, the bound that holds against quotients of different bits
(tests/test_census_se_cpu.py).
A score row takes test_gpu_census.py's acc bound with the barcode's own counts: 2^-52 (T_b + V + 8) score_bv, T_b = reads_b + 2 pairs_b.
The identities sum_u H_vu w_u = acc_v and w' H w = N hold within these bounds plus the V + 1 roundings of the product with w."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import census_ref as R
import census_se_ref as SE

pytestmark = pytest.mark.gpu
U = R.U
TRUE8 = np.array([.4, .25, .15, .1, .05, .03, .02, 0.0])


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import build, capi, census, engine, refine, synth
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    mat, err = engine.phred_tables()
    return dict(torch=torch, capi=capi, engine=engine, refine=refine, synth=synth, census=census, mat=mat, err=err)


def open_engine(m, g, pl):
    e = m["engine"].Engine(g.shape[1], (0.0, 0.5), 0.5)
    e.set_genotypes(g); e.set_pileup(pl)
    return e


def make_case(m, seed, B, S, V, n_reads, shares=None, **kw):
    rng = np.random.default_rng(seed)
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = R.gt_rows(raw.alleles, 0.01)
    shares = rng.dirichlet(np.ones(V)) if shares is None else shares
    pl = R.make_pool(rng, raw.alleles, shares, B, n_reads, **kw)
    return rng, g, pl


def share_kinds(rng, V, G):
    out = {"uniform": np.full((G, V), 1.0 / V), "dirichlet": rng.dirichlet(np.ones(V), size=G)}
    if V >= 2:
        z = rng.dirichlet(np.ones(V), size=G)
        z[:, rng.choice(V, max(1, V // 3), replace=False)] = 0.0
        z[:, 0] += 1e-3                                  # (never an all-zero row)
        out["zeros"] = z / z.sum(axis=1, keepdims=True)
    return out


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def same_bits(a, b, keys=("H", "score", "n_read_b", "acc", "ll", "n_read", "n_pair")):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


def check_identities(got, k, w, label=""):
    """sum_u H_vu w_u = acc_v and w' H w = N for group k, within the H and acc bounds and the product's own roundings."""
    V = len(w)
    H, acc, N, P = got["H"][k], got["acc"][k], float(got["n_read"][k]), float(got["n_pair"][k])
    T = N + 2 * P
    Hw = H @ w
    tol = U * (P + 16) * Hw + U * (V + 1) * Hw + U * (T + V + 8) * acc
    assert np.all(np.abs(Hw - acc) <= tol), (label, k, float(np.max(np.abs(Hw - acc) / np.maximum(tol, 1e-300))))
    assert abs(float(w @ Hw) - N) <= U * ((P + 16) + 2 * (V + 1) + (T + V + 8)) * N, (label, k)


def check_group(m, got, k, fl, d, valid, group, w, label="", only=None):
    """Group k of a census_fisher result against the restatement; prints measured / bound.  `only`: the rows of H that the restatement
    forms and that are compared (None = all); the score rows and the counts are always compared whole."""
    V = d.shape[1]
    member = np.asarray(group) == k
    ref = SE.fisher(fl, d, valid, member, w, m["mat"], m["err"], only=only)
    assert got["n_read"][k] == ref.n_read and got["n_pair"][k] == ref.n_pair, (label, k)
    H = got["H"][k]
    assert np.array_equal(H, H.T), (label, k)
    sel = slice(None) if only is None else np.asarray(only)
    tol_H = U * (ref.n_pair + 16) * ref.H[sel]
    dH = np.abs(H[sel] - ref.H[sel])
    Tb = (ref.n_read_b + 2 * ref.n_pair_b)[:, None]
    tol_s = U * (Tb + V + 8) * ref.score
    ds = np.abs(got["score"][member] - ref.score[member])
    r_H = float(np.max(dH / np.maximum(tol_H, 1e-300))) if ref.n_pair else 0.0
    r_s = float(np.max(ds / np.maximum(tol_s[member], 1e-300))) if ref.n_pair else 0.0
    print(f"{label} group {k}: N {ref.n_read} pairs {ref.n_pair} max d H / bound {r_H:.3f} max d score / bound {r_s:.3f}")
    assert np.all(dH <= tol_H), (label, k, r_H)
    assert np.all(ds <= tol_s[member]), (label, k, r_s)
    assert np.array_equal(got["n_read_b"][member], ref.n_read_b[member]), (label, k)
    # the barcodes' rows add up to the group's acc, within the acc bound
    T = ref.n_read + 2 * ref.n_pair
    assert np.all(np.abs(got["score"][member].sum(axis=0, dtype=np.longdouble).astype(np.float64) - got["acc"][k]) <= U * (T + V + 8) * got["acc"][k]), (label, k)
    if not ref.n_read:
        assert not H.any() and not got["score"][member].any()
    return ref


@pytest.mark.parametrize("B,S,V,n_reads,G", [
    (50, 500, 1, 4000, 1),
    (120, 1500, 2, 15000, 2),
    (300, 4000, 11, 30000, 3),         # E = 66: the second 64-lane slot holds two entries
    (100, 800, 33, 12000, 2),
    (80, 700, 63, 10000, 1),           # E = 2016: one entry block, not full
    (100, 800, 64, 10000, 1),          # E = 2080: the second entry block holds 32 entries
    (80, 700, 65, 10000, 2),           # E = 2145
    (60, 600, 128, 10000, 1),          # the cap: E = 8256, five entry blocks
])
def test_fisher_against_the_restatement(m, B, S, V, n_reads, G):
    """Uniform, Dirichlet and zero-holding shares, some barcodes at -1.  Every kind is checked for symmetry, both identities, the score
    sums and census_step's bits, and entry by entry against the restatement: all of H at V <= 33 and for the zero-holding kind (which is
    Dirichlet elsewhere); at V >= 63, where a whole H costs the restatement seconds per call, the other two kinds are compared on eight
    rows of H, which between them hold entries of every entry block (row v of the symmetric H holds the upper-triangle entries (u, v),
    u < v, and (v, u), u >= v), and on all score rows."""
    rng, g, pl = make_case(m, 200 * V + G, B, S, V, n_reads)
    fl = R.flatten(pl)
    d, valid = R.dosage(g)
    group = rng.integers(0, G, B).astype(np.int32)
    group[rng.random(B) < 0.1] = -1
    E = V * (V + 1) // 2
    some = sorted({0, 1, V // 4, V // 2 - 1, V // 2, 3 * V // 4, V - 2, V - 1})
    e = open_engine(m, g, pl)
    try:
        for kind, w in share_kinds(rng, V, G).items():
            got = e.census_fisher(group, w, n_groups=G)
            step = e.census_step(group, w, n_groups=G)
            assert all(np.array_equal(bits(got[n]), bits(x)) for n, x in zip(("acc", "ll", None, "n_read", "n_pair"), step) if n), kind
            assert not got["score"][group < 0].any() and not got["n_read_b"][group < 0].any()
            for k in range(G):
                assert np.array_equal(got["H"][k], got["H"][k].T) and (got["H"][k] >= 0).all()
                check_identities(got, k, w[k], f"V={V} {kind}")
                assert got["n_read_b"][group == k].sum() == got["n_read"][k]
                check_group(m, got, k, fl, d, valid, group, w[k], f"V={V} {kind}", only=None if V <= 33 or kind == "zeros" else some)
        info = e.census_fisher_info()
    finally:
        e.close()
    assert info["n_groups"] == G and info["n_samples"] == V and info["n_cells"] == B and info["n_entries"] == E
    assert info["n_blocks"] == (E + 2047) // 2048 and info["n_chunks"] >= G and info["partial_bytes"] == info["n_chunks"] * E * 8
    assert info["kernel_ms"] > 0.0


def test_bits(m):
    torch = m["torch"]
    rng, g, pl = make_case(m, 13, 200, 1200, 12, 25000)
    V, G, B = 12, 5, 200
    fl = R.flatten(pl)
    d, valid = R.dosage(g)
    group = rng.integers(-1, G, B).astype(np.int32)
    w = rng.dirichlet(np.ones(V), size=G)
    a = rng.uniform(0.05, 0.95, size=1200)
    assign = rng.integers(0, V, B).astype(np.int32)
    e = open_engine(m, g, pl)
    try:
        r1 = e.census_fisher(group, w)
        assert same_bits(r1, e.census_fisher(group, w))                                        # a repeat
        d_group = torch.from_numpy(group).to("cuda:0")
        assert same_bits(r1, e.census_fisher(int(d_group.data_ptr()), w, n_groups=G))          # a device group
        for k in range(G):                                                                  # a group alone
            alone = e.census_fisher(np.where(group == k, 0, -1).astype(np.int32), w[k:k + 1])
            assert np.array_equal(bits(r1["H"][k]), bits(alone["H"][0])), k
            assert np.array_equal(bits(r1["score"][group == k]), bits(alone["score"][group == k])), k
            assert np.array_equal(bits(r1["acc"][k]), bits(alone["acc"][0])) and r1["ll"][k] == alone["ll"][0]
        # a barcode's score row depends on its own pairs and its w row only: every barcode in one group with w[2], shuffled chunks
        one = e.census_fisher(np.zeros(B, dtype=np.int32), w[2:3])
        two = e.census_fisher((np.arange(B) % 3).astype(np.int32), np.repeat(w[2:3], 3, axis=0))
        assert np.array_equal(bits(one["score"]), bits(two["score"])) and np.array_equal(one["n_read_b"], two["n_read_b"])
        assert np.array_equal(bits(one["score"][group == 2]), bits(r1["score"][group == 2]))
        c1 = e.census(group, n_groups=G)
        ci = e.census_info()
        e.run(); e.sync()
        llks, llk0s = e.get_singlet()
        amb = e.ambient_profile(assign, a, np.array([0.0, 0.1, 0.3]))
        assert same_bits(r1, e.census_fisher(group, w))                                        # after run() and ambient_profile
        # ... and the call leaves the other results as they were
        l2, l02 = e.get_singlet()
        assert np.array_equal(bits(llks), bits(l2)) and np.array_equal(bits(llk0s), bits(l02))
        ll = np.zeros_like(amb[0]); ns = np.zeros_like(amb[1]); nr = np.zeros_like(amb[2])
        m["capi"].check(e._L.dmx_engine_get_ambient(e._h, ll.ctypes.data, ns.ctypes.data, nr.ctypes.data))
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(amb, (ll, ns, nr)))
        wq = np.zeros((G, V)); llq = np.zeros(G)
        m["capi"].check(e._L.dmx_engine_get_census(e._h, wq.ctypes.data, llq.ctypes.data, None, None, None, None, None))
        assert np.array_equal(bits(wq), bits(c1["w"])) and np.array_equal(bits(llq), bits(c1["ll"]))
        assert e.census_info() == ci
    finally:
        e.close()
    # read-count widths: the same bits; dense against sparse: within the bounds
    res = {}
    for name, p in (("sparse", pl), ("dense", R.to_dense(pl))):
        for width in (1, 2, 4):
            q = m["engine"].HostPileup(p.n_cells, p.n_snps, p.cell_pair_off, p.cell_read_off, p.pair_snp,
                                       np.asarray(p.pair_nrd).astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[width]), p.reads, p.rd_totl,
                                       p.rd_pass, p.rd_uniq)
            e = open_engine(m, g, q)
            try:
                res[name, width] = e.census_fisher(group, w)
            finally:
                e.close()
    assert same_bits(res["sparse", 1], r1)
    for name in ("sparse", "dense"):
        for width in (2, 4):
            assert same_bits(res[name, 1], res[name, width]), (name, width)
    for k in range(G):
        check_group(m, res["dense", 1], k, fl, d, valid, group, w[k], "dense")


def edge_case(m):
    """Barcode 0: no pair; 1: one pair of one read; 2: 64 pairs (one full tile); 3: 65 pairs, SNP 7 among them; 4: a pair of 255 reads and
    a pair of 9; 5: a pair without stored reads and a normal one; 6, 7: a few reads each.  SNP 7 has an all-zero row for donor 2."""
    rng = np.random.default_rng(11)
    S, V, B = 260, 4, 8
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = R.gt_rows(raw.alleles, 0.01)
    g[7, 2] = 0.0
    cell, snp, byte = [], [], []

    def add(c, s, al, bq):
        cell.append(c); snp.append(s); byte.append((al << 7) | bq)
    add(1, 55, 0, 37)
    for s in range(100, 164):
        add(2, s, int(rng.integers(0, 2)), int(rng.integers(10, 41)))
    for s in range(65):
        add(3, s, int(rng.integers(0, 2)), int(rng.integers(10, 41)))
    for _ in range(255):
        add(4, 100, int(rng.random() < 0.4), int(rng.integers(10, 41)))
    for _ in range(9):
        add(4, 20, int(rng.integers(0, 2)), int(rng.integers(10, 41)))
    add(5, 31, 1, 30)
    for c in (6, 7):
        for s in rng.choice(S, 6, replace=False):
            add(c, int(s), int(rng.integers(0, 2)), int(rng.integers(10, 41)))
    pl = R.build_pileup(B, S, cell, snp, byte, nrd_dtype=np.uint8, extra_pairs=[(5, 30)])
    return rng, g, pl


def test_edges(m):
    rng, g, pl = edge_case(m)
    fl = R.flatten(pl)
    assert np.diff(pl.cell_pair_off).tolist()[:6] == [0, 1, 64, 65, 2, 2] and fl.nrd.max() == 255 and (fl.nrd == 0).sum() == 1
    d, valid = R.dosage(g)
    assert (~valid).sum() == 1 and not valid[7]
    V, G = 4, 6
    group = np.array([3, 0, 1, 1, 2, 2, 4, -1], dtype=np.int32)       # group 3 is the barcode without a pair, group 5 has no barcode
    w = rng.dirichlet(np.ones(V), size=G)
    e = open_engine(m, g, pl)
    try:
        got = e.census_fisher(group, w, n_groups=G)
        for k in range(G):
            check_group(m, got, k, fl, d, valid, group, w[k], "edges")
            check_identities(got, k, w[k], "edges")
        for k in (3, 5):                                              # no counted read: H = 0, scores 0
            assert not got["H"][k].any() and got["n_read"][k] == 0 and not got["acc"][k].any() and got["ll"][k] == 0.0
        assert not got["score"][0].any() and not got["score"][7].any()
        assert got["n_read_b"].tolist()[:6] == [0, 1, 64, 64, 264, 1]  # barcode 3 without the pair at the invalid SNP, 5 without the empty pair
        assert got["n_pair"].tolist()[:4] == [1, 128, 3, 0] and got["n_pair"][5] == 0
        none = e.census_fisher(np.full(8, -1, dtype=np.int32), w[:2], n_groups=2)   # every barcode unused
        assert not none["H"].any() and not none["score"].any() and not none["n_read_b"].any() and not none["n_read"].any()
        # any output may be NULL
        capi = m["capi"]
        H = np.zeros((G, V, V))
        rq = capi.CensusFisherRequest(8, capi.DMX_MEM_HOST, group.ctypes.data, G, V, w.ctypes.data, H.ctypes.data)
        capi.check(e._L.dmx_engine_census_fisher(e._h, C.byref(rq)))
        assert np.array_equal(bits(H), bits(got["H"]))
        rq = capi.CensusFisherRequest(8, capi.DMX_MEM_HOST, group.ctypes.data, G, V, w.ctypes.data)
        capi.check(e._L.dmx_engine_census_fisher(e._h, C.byref(rq)))
    finally:
        e.close()


def test_argument_errors(m):
    capi = m["capi"]
    rng, g, pl = make_case(m, 19, 20, 100, 4, 800)
    V, B = 4, 20
    w = np.full((2, V), 0.25)
    grp = (np.arange(B) % 2).astype(np.int32)

    def raises(code, fn, *a, **k):
        with pytest.raises(capi.DmxError) as ei:
            fn(*a, **k)
        assert ei.value.code == code, ei.value

    e = m["engine"].Engine(V, (0.0, 0.5), 0.5)
    try:
        e.B = 3                                                             # an empty pileup is staged, but no genotype matrix yet
        z = np.zeros(3, dtype=np.int32)
        e.set_pileup(m["engine"].HostPileup(3, 0, np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32),
                                            np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), z, z.copy(), z.copy()))
        raises(-3, e.census_fisher, np.zeros(3, dtype=np.int32), w[:1])
    finally:
        e.close()
    e = m["engine"].Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g)
        e.B = B
        raises(-3, e.census_fisher, grp, w)                                 # genotypes, but no pileup yet
        e.set_pileup(pl)
        raises(-3, e.census_fisher_info)                                    # nothing computed yet
        raises(-1, e.census_fisher, grp, np.full((1025, V), 0.25), n_groups=1025)
        raises(-1, e.census_fisher, grp, np.zeros((0, V)), n_groups=0)
        raises(-1, e.census_fisher, np.full(B, 2, dtype=np.int32), w, n_groups=2)          # group[b] = G
        raises(-1, e.census_fisher, np.full(B, -2, dtype=np.int32), w, n_groups=2)
        for bad in (np.array([[0.5, 0.5, 0.5, -0.5]] * 2), np.full((2, V), 0.26), np.array([[np.nan, 1, 0, 0]] * 2),
                    np.array([[1.0, 0, 0, 0], [0.25, 0.25, 0.25, 0.25 + 1e-9]])):
            raises(-1, e.census_fisher, grp, bad)
        rq = capi.CensusFisherRequest(B + 1, capi.DMX_MEM_HOST, grp.ctypes.data, 2, V, w.ctypes.data)
        assert e._L.dmx_engine_census_fisher(e._h, C.byref(rq)) == -1                # n_cells does not match
        rq = capi.CensusFisherRequest(B, capi.DMX_MEM_HOST, grp.ctypes.data, 2, V + 1, w.ctypes.data)
        assert e._L.dmx_engine_census_fisher(e._h, C.byref(rq)) == -1                # n_samples does not match
        rq = capi.CensusFisherRequest(B, 7, grp.ctypes.data, 2, V, w.ctypes.data)
        assert e._L.dmx_engine_census_fisher(e._h, C.byref(rq)) == -1                # group_memory
        rq = capi.CensusFisherRequest(B, capi.DMX_MEM_HOST, None, 2, V, w.ctypes.data)
        assert e._L.dmx_engine_census_fisher(e._h, C.byref(rq)) == -1                # no group
        rq = capi.CensusFisherRequest(B, capi.DMX_MEM_HOST, grp.ctypes.data, 2, V, None)
        assert e._L.dmx_engine_census_fisher(e._h, C.byref(rq)) == -1                # no w
        assert e._L.dmx_engine_census_fisher(e._h, None) == -1 and e._L.dmx_engine_census_fisher_info(e._h, None) == -1
        raises(-3, e.census_fisher_info)                                    # still nothing computed
        with pytest.raises(ValueError):
            e.census_fisher(np.zeros(B + 1, dtype=np.int32), w)
        with pytest.raises(ValueError):
            e.census_fisher(grp, np.full((2, V + 1), 0.2))
        got = e.census_fisher(grp, w)                                       # and the engine still works
        assert got["n_read"].sum() == len(pl.reads) and e.census_fisher_info()["n_groups"] == 2
    finally:
        e.close()
    # V = 129: one donor more than the cap
    rng, g, pl = make_case(m, 23, 6, 40, 129, 300)
    e = open_engine(m, g, pl)
    try:
        raises(-1, e.census_fisher, np.zeros(6, dtype=np.int32), np.full((1, 129), 1.0 / 129))
        assert e.census_step(np.zeros(6, dtype=np.int32), np.full((1, 129), 1.0 / 129))[3][0] == len(pl.reads)     # (the step has no such cap)
    finally:
        e.close()


def test_nomem_at_the_cap(m):
    """DMX_ERR_NOMEM at V = 128: an empty pileup of so many barcodes that the chunk partials (E x 8 bytes per chunk of 4 barcodes) and the
    score rows (V x 8 bytes per barcode) exceed the free device memory is refused before the call allocates anything of its own, and a
    small call on the same engine is right afterwards."""
    capi, eng = m["capi"], m["engine"]
    V, S, B = 128, 80, 12
    rng, g, pl = make_case(m, 29, B, S, V, 600)
    E = V * (V + 1) // 2
    free = m["torch"].cuda.mem_get_info(0)[0]
    nb = int(free // (2 * E + 8 * V)) + 1024                # 2 E + 8 V bytes per barcode: more than the memory that is free now
    assert nb < 2 ** 31 - 2 ** 27 and (nb + 3) // 4 * 5 < 2 ** 31 - 4
    po = np.zeros(nb + 1, dtype=np.int64)
    zi = np.zeros(nb, dtype=np.int32)
    w = np.full((1, V), 1.0 / V)
    e = eng.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g)
        e.set_pileup(eng.HostPileup(nb, S, po, po, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), zi, zi, zi))
        rq = capi.CensusFisherRequest(nb, capi.DMX_MEM_HOST, zi.ctypes.data, 1, V, w.ctypes.data)      # every barcode in group 0, no output asked for
        with pytest.raises(capi.DmxError) as ei:
            capi.check(e._L.dmx_engine_census_fisher(e._h, C.byref(rq)))
        assert ei.value.code == capi.DMX_ERR_NOMEM == -6 and f"of {E} entries" in str(ei.value)     # this call's own check, not the plan's
        with pytest.raises(capi.DmxError) as ei:
            e.census_fisher_info()                                                                     # nothing was computed
        assert ei.value.code == -3
        e.set_pileup(pl)
        group = (np.arange(B) % 2).astype(np.int32)
        w2 = rng.dirichlet(np.ones(V), size=2)
        got = e.census_fisher(group, w2)
        info = e.census_fisher_info()
    finally:
        e.close()
    assert info["n_blocks"] == 5 and info["n_cells"] == B
    fl = R.flatten(pl)
    d, valid = R.dosage(g)
    for k in range(2):
        check_group(m, got, k, fl, d, valid, group, w2[k], "after NOMEM")
        check_identities(got, k, w2[k], "after NOMEM")


def test_gap_on_support(m):
    """Flag 0: the driver's results are bit-identical to a call that never sets it.  With the flag and a zeroed donor the driver takes
    the restatement's driver's passes and reaches its shares.  The donors zeroed are 4 and 6 (fitted shares 0.044 and 0.014): a small
    change of the fit, refitted in a few dozen passes along which the device's and the restatement's roundings (~1e-13 relative per
    pass) do not grow, so the pass counts are equal and 1e-9 is asked of the shares.  (A refit without a large donor takes over a
    hundred SQUAREM passes whose step lengths and LL comparisons turn on the last bits; the restatement's own pass count moves
    by a few when its start is changed by 1e-13 there, so equality of counts would say nothing.)  Without the flag the same refit runs
    into max_steps."""
    rng, g, pl = make_case(m, 17, 90, 1500, 8, 14000, shares=TRUE8)
    fl = R.flatten(pl)
    d, valid = R.dosage(g)
    B, V = 90, 8
    group = np.zeros(B, dtype=np.int32)
    capi = m["capi"]
    e = open_engine(m, g, pl)
    try:
        full = e.census(group, n_groups=1)
        off = e.census(group, n_groups=1, gap_on_support=False)
        assert all(np.array_equal(bits(full[n]), bits(off[n])) for n in full)
        rq = capi.CensusRequest(B, capi.DMX_MEM_HOST, group.ctypes.data, 1, V, None, 1e-4, 2000, 1)      # the struct as an older caller fills it
        capi.check(e._L.dmx_engine_census(e._h, C.byref(rq)))
        wq = np.zeros((1, V))
        capi.check(e._L.dmx_engine_get_census(e._h, wq.ctypes.data, None, None, None, None, None, None))
        assert np.array_equal(bits(wq), bits(full["w"]))
        on_full = e.census(group, n_groups=1, gap_on_support=True)             # a uniform start: every donor is in the support
        assert all(np.array_equal(bits(full[n]), bits(on_full[n])) for n in full)
        w0 = {v: m["census"].presence_start(full["w"], v) for v in (4, 6)}
        on = {v: e.census(group, n_groups=1, w0=w0[v], gap_on_support=True) for v in (4, 6)}
        stuck = e.census(group, n_groups=1, w0=w0[4], max_steps=300)
    finally:
        e.close()
    for v in (4, 6):
        ref = SE.run(fl, d, valid, group == 0, m["mat"], m["err"], w0=w0[v][0], gap_on_support=True)
        print(f"refit without donor {v}: passes", int(on[v]["n_steps"][0]), "restatement", ref["n_steps"], "max |d w|",
              float(np.max(np.abs(on[v]["w"][0] - ref["w"]))))
        assert on[v]["converged"][0] == 1 and on[v]["gap"][0] <= 1e-4 and on[v]["n_steps"][0] == ref["n_steps"] < 200
        assert on[v]["w"][0, v] == 0.0 and np.max(np.abs(on[v]["w"][0] - ref["w"])) <= 1e-9
        assert abs(on[v]["ll"][0] - ref["ll"]) <= 1e-6 and on[v]["ll"][0] < full["ll"][0]
    print("without the flag: passes", int(stuck["n_steps"][0]), "gap", float(stuck["gap"][0]))
    assert stuck["n_steps"][0] == 300 and stuck["converged"][0] == 0 and stuck["gap"][0] > 1.0


def test_presence_calls_on_the_recovery_pool(m):
    """census_run(presence=True, se=True) on the recovery pool of test_gpu_census.py: the calls of tests/test_census_se_cpu.py (the donor
    of true share 0.03 found with P < 1e-3, the absent donor not: P > 0.1; the 0.02 donor not asserted), every refit converged in far
    fewer than max_steps passes, and the standard errors finite and positive for the free donors."""
    rng = np.random.default_rng(2201)
    raw = m["synth"].make_raw_genotypes(rng, 4000, 8)
    g = R.gt_rows(raw.alleles, 0.01)
    pl = R.make_pool(rng, raw.alleles, TRUE8, 300, 40000)
    r = m["census"].census_run(pl, g, [f"S{j}" for j in range(8)], None, se=True, presence=True)
    p = r["presence"]
    print("P", p["p"][0], "LLR", p["llr"][0].round(2), "steps", p["n_steps"][0], "SE", r["cov"][0]["se"].round(4), "robust", r["cov"][0]["se_robust"].round(4))
    assert p["p"][0, 5] < 1e-3 and p["p"][0, 7] > 0.1 and (p["p"][0, :5] < 1e-6).all()
    assert (p["converged"] == 1).all() and p["n_steps"].max() < 200
    c = r["cov"][0]
    F = c["free"]
    assert set(range(6)) <= set(F.tolist()) and (c["se"][F] > 0).all() and (c["se_robust"][F] > 0).all() and np.isfinite(c["se_robust"][F]).all()
    assert np.all(np.abs(r["w"][0, :6] - TRUE8[:6]) <= 4.0 * np.maximum(c["se"][:6], c["se_robust"][:6]) + 0.005)   # (independent reads: either SE is right; 0.005 for the 1 % genotype error)


def test_census_run_end_to_end(m, tmp_path):
    """--se --presence on a `demuxlet --pileup-only` dump: the three earlier files keep their bytes, the new files parse, and the SEs agree
    with census_se_ref's at the fitted shares within cond(G1) x the H bound x 10 (a relative perturbation of G1 moves its inverse by at most
    cond(G1) times as much, to first order; 10 for the rest of the linear algebra); the test computes cond(G1)."""
    import sam_vcf_synth as sv
    census = m["census"]
    cli = Path(census.__file__).resolve().parent / "demuxlet"
    contigs = [("1", 30000), ("2", 20000)]
    samples = ["smC", "smA", "smB", "smD"]
    rng = np.random.default_rng(23)
    recs = sv.make_vcf(rng, contigs, 120, samples, tmp_path / "v.vcf.gz")
    bcs = [f"BC{i:02d}-1" for i in range(25)]
    sv.make_reads(rng, contigs, recs, 4000, bcs, tmp_path / "r.sam", tmp_path / "r.bam")
    subprocess.run([str(cli), "--sam", str(tmp_path / "r.sam"), "--vcf", str(tmp_path / "v.vcf.gz"), "--field", "GT", "--out", str(tmp_path / "o"),
                    "--pileup-only"], check=True, stderr=subprocess.DEVNULL)
    dump = str(tmp_path / "o.pileup.txt")
    dd = m["refine"].read_pileup_txt(dump)
    V = len(dd.sample_ids)
    (tmp_path / "g.tsv").write_text("".join(f"{b}\t{'odd' if i % 2 else 'even'}\n" for i, b in enumerate(dd.barcodes[:-3])))
    assert census.main(["--pileup", dump, "--out", str(tmp_path / "a"), "--groups", str(tmp_path / "g.tsv")]) == 0
    assert census.main(["--pileup", dump, "--out", str(tmp_path / "b"), "--groups", str(tmp_path / "g.tsv"), "--se", "--presence"]) == 0
    for ext in (".census.tsv", ".census_groups.tsv", ".census_profile.tsv"):
        assert (tmp_path / ("a" + ext)).read_bytes() == (tmp_path / ("b" + ext)).read_bytes(), ext
    for ext in (".census_se.tsv", ".census_cov.tsv", ".census_presence.tsv"):
        assert not (tmp_path / ("a" + ext)).exists() and (tmp_path / ("b" + ext)).exists(), ext
    r = census.census_run(dd.pileup, dd.g, dd.sample_ids, None, groups=str(tmp_path / "g.tsv"), barcodes=dd.barcodes, se=True, presence=True)
    names = ["even", "odd"]
    assert r["names"] == names
    rows = [x.split("\t") for x in (tmp_path / "b.census_se.tsv").read_text().splitlines()]
    assert rows[0] == census.SE_HEADER.rstrip("\n").split("\t") and len(rows) == 1 + 2 * V
    prow = [x.split("\t") for x in (tmp_path / "b.census_presence.tsv").read_text().splitlines()]
    assert prow[0] == census.PRESENCE_HEADER.rstrip("\n").split("\t") and len(prow) == 1 + 2 * V
    crow = [x.split("\t") for x in (tmp_path / "b.census_cov.tsv").read_text().splitlines()]
    assert crow[0] == census.COV_HEADER.rstrip("\n").split("\t")
    fl = R.flatten(dd.pileup)
    d, valid = R.dosage(dd.g)
    for k, name in enumerate(names):
        member = r["group"] == k
        ref = SE.fisher(fl, d, valid, member, r["w"][k], m["mat"], m["err"])
        se, se_r, bound = SE.covariance(ref.H, r["w"][k], ref.n_read, ref.score[member], ref.n_read_b[member])
        c = r["cov"][k]
        F = c["free"]
        assert np.array_equal(bound, c["at_bound"]) and len(F) >= 2
        Q = census.sum_zero_basis(len(F))
        cond = float(np.linalg.cond(Q.T @ ref.H[np.ix_(F, F)] @ Q))
        tol = cond * U * (ref.n_pair + 16) * 10
        print(f"{name}: cond(G1) {cond:.3g}, SE {c['se'].round(4)} robust {c['se_robust'].round(4)}, max relative difference "
              f"{np.max(np.abs(c['se'][F] - se[F]) / se[F]):.3g} / {np.max(np.abs(c['se_robust'][F] - se_r[F]) / se_r[F]):.3g}, bound {tol:.3g}")
        assert np.all(np.abs(c["se"][F] - se[F]) <= tol * se[F]) and np.all(np.abs(c["se_robust"][F] - se_r[F]) <= tol * se_r[F])
        assert len([x for x in crow[1:] if x[0] == name]) == len(F) * (len(F) + 1) // 2
        for v, sid in enumerate(dd.sample_ids):
            x = rows[1 + k * V + v]
            assert x[:2] == [name, sid] and x[2] == format(r["w"][k, v], ".6f") and x[3] == format(c["se"][v], ".6f") and int(x[7]) == int(c["at_bound"][v])
            if np.isfinite(c["se_robust"][v]):
                assert x[4] == format(c["se_robust"][v], ".6f") and 0.0 <= float(x[5]) <= float(x[2]) <= float(x[6]) <= 1.0
            else:
                assert x[4:7] == ["NA", "NA", "NA"]
            y = prow[1 + k * V + v]
            assert y[:3] == x[:3] and float(y[5]) >= 0.0 and 0.0 <= float(y[6]) <= 1.0 and int(y[8]) == 1
            if c["at_bound"][v]:
                assert y[5:8] == ["0.00000", "1", "0"]
            else:
                assert float(y[5]) == pytest.approx(max(float(y[3]) - float(y[4]), 0.0), abs=2e-5) and int(y[7]) >= 1
