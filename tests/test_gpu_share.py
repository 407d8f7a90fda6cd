"""GPU (-m gpu): the continuous mixing share (Engine.share_scan / share_fit, dmx_engine_share_scan / _share_fit; share.share_run).

Against the long double restatement of tests/share_ref.py, with U = 2^-52, N the barcode's counted pairs, R its counted reads and n_max
its deepest pair:
  LL    |d| <= U (N + 3) sum|lg| + 1.12 U sum|lg|: DESIGN.md section 22's form (N serial adds and dmx_log's 1.12 ulp).  The form leaves
        out the roundings of the log's argument (L carries 4 n + 10 of them, which the log passes on as an absolute error), so a barcode
        of very few pairs comes closest to it; the share is therefore printed for N >= 63 and for N < 63 apart.
  LL'   |d| <= U k1 m1,  k1 = 9 n_max + 20 + N + 63: per pair the numerator takes n + 5 (u: three roundings of t, one of pA - pR, one
        quotient; n - 1 adds; the product with s), 4 n for T, 1 for T x and 5 adds; L takes 4 n + 8; one quotient; then at most
        N + 63 adds over the pairs in either summation plan.  m1 = sum_i sum_lm T |s| sum_r|u| / L (share_ref's m1).
  LL''  |d| <= U k2 m2,  k2 = 2 (9 n_max + 20) + 2 + N + 63: D1 D1 doubles D1's count, plus the product and the difference; the L'' / L
        part needs less (10 n + 27).  m2 = sum_i (A2_i + A1_i^2) (share_ref's m2).
The fit: status and evaluation count equal the restated driver's unless one of its branch decisions was within 1e-9 of its boundary (at
most 2 % of the cases); LL(alpha_hat) >= LL(alpha*) - 1e-9 and, where -LL''(alpha*) >= 1, |alpha_hat - alpha*| <= 2 tol, alpha* by
bisection in long double; LL at alpha_hat, 0 and 1 against dmx_engine_ambient_doublet, which sums in another order.  Then the bits, every
error code, the recovery of unequal doublets that the plain pass calls SNG-, and the command line.

Recovery, measured on the MI355X (seed 2806): see test_recovery_of_unequal_doublets's docstring."""
import numpy as np
import pytest

import share_ref as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -52
SPECIAL = (0, 1, 63, 64, 65, 200)          # pairs of the first six barcodes: the tile's edges


@pytest.fixture(scope="module")
def m():
    from demuxlet_amd import ambient, build, capi, engine, refine, share, synth
    build.build()
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    capi.load()
    return dict(torch=torch, capi=capi, engine=engine, refine=refine, synth=synth, ambient=ambient, share=share)


def host_pileup(m, sp, width=None):
    nrd = np.asarray(sp.pair_nrd)
    if width is not None:
        nrd = nrd.astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[width])
    return m["engine"].HostPileup(sp.n_cells, sp.n_snps, sp.cell_pair_off, sp.cell_read_off, sp.pair_snp, nrd, sp.reads,
                                  sp.rd_totl, sp.rd_pass, sp.rd_uniq)


def genotypes(m, rng, S, V, soft):
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    if soft:
        g = np.stack([m["engine"].geno_from_gp(x, 0.01) for x in m["synth"].raw_gp_from_alleles(rng, raw.alleles)])
    else:
        g = np.zeros((S, V, 3), dtype=np.float32)
        dos = np.clip(raw.alleles, 0, 1).sum(axis=2)
        for k in range(3):
            g[:, :, k] = dos == k                                     # one-hot rows
    g[rng.choice(S, S // 12, replace=False), rng.integers(0, V)] = 0.0   # all-zero rows
    return raw, g


def make_problem(m, seed, V, soft, dense=False, deep=True):
    """B = 48 barcodes over S = 400 SNPs (dense: 6 over 130): the first six hold SPECIAL's pairs, pairs carry 0 - 20 reads (both sides of
    the rescaling's 8), barcode 5 one pair of 300 reads; barcode b is a doublet of donors (b mod V, (b + 1) mod V) at share 0.1 - 0.4."""
    rng = np.random.default_rng(seed)
    B, S = (6, 130) if dense else (48, 400)
    raw, g = genotypes(m, rng, S, V, soft)
    dos = np.clip(raw.alleles, 0, 1).sum(axis=2) / 2.0
    po, snps, nrds, reads = [0], [], [], []
    truth = np.zeros((B, 2), dtype=np.int32)
    for b in range(B):
        n = S if dense else (SPECIAL[b] if b < len(SPECIAL) else int(rng.integers(20, 260)))
        sn = np.arange(S) if dense else np.sort(rng.choice(S, n, replace=False))
        nr = rng.integers(0, 4, size=n) if dense else np.where(rng.random(n) < 0.1, 0, rng.integers(1, 21, size=n))
        if deep and b == 5:
            nr[n // 2] = 300
        v1, v2, al = b % V, (b + 1) % V, rng.uniform(0.1, 0.4)
        truth[b] = (v1, v2)
        for s_, k in zip(sn, nr):
            src = np.where(rng.random(k) < al, v2, v1)
            alt = rng.random(k) < dos[s_, src]
            bq = rng.integers(2, 41, size=k)
            flip = rng.random(k) < 10.0 ** (-bq / 10.0)
            reads.append((((alt ^ flip).astype(np.uint8)) << 7 | bq.astype(np.uint8)).astype(np.uint8))
        snps.append(sn); nrds.append(nr); po.append(po[-1] + n)
    nrd = np.concatenate(nrds)
    rd = np.concatenate(reads) if reads else np.zeros(0, dtype=np.uint8)
    po = np.array(po, dtype=np.int64)
    ro = np.concatenate([[0], np.cumsum(nrd)])[po]
    t = np.ones(B, dtype=np.int32)
    sp = m["synth"].SynthPileup(B, S, po, ro.astype(np.int64), None if dense else np.concatenate(snps).astype(np.int32),
                                nrd.astype(np.uint16 if deep else np.uint8), rd, t, t, t, truth)
    a = rng.uniform(0.02, 0.98, size=S)
    return dict(sp=sp, g=g, a=a, truth=truth, B=B, S=S, V=V, rng=rng)


def candidates(p, C):
    """cand[B][C][2]: the true pair, the true pair swapped, then random pairs; every seventh barcode's last slot unused."""
    rng, B, V = np.random.default_rng(5), p["B"], p["V"]
    cand = np.full((B, C, 2), -1, dtype=np.int32)
    for b in range(B):
        for c in range(C):
            if c == 0:
                cand[b, c] = p["truth"][b]
            elif c == 1:
                cand[b, c] = p["truth"][b][::-1]
            else:
                v1 = int(rng.integers(0, V))
                cand[b, c] = (v1, (v1 + 1 + int(rng.integers(0, V - 1))) % V)
        if b % 7 == 6:
            cand[b, C - 1] = -1
    return cand


def engine_for(m, p, width=None):
    e = m["engine"].Engine(p["V"], (0.0, 0.5), 0.5)
    e.set_genotypes(p["g"]); e.set_pileup(host_pileup(m, p["sp"], width))
    return e


def bounds(ev):
    N, n = ev.n_snp, ev.n_max
    b22 = U * (N + 3) * ev.abs_lg + 1.12 * U * ev.abs_lg
    return b22, U * (9 * n + 20 + N + 63) * ev.m1, U * (2 * (9 * n + 20) + 2 + N + 63) * ev.m2


class Shares:
    """Largest measured share of each bound."""
    def __init__(self):
        self.s = dict(ll=0.0, ll_small=0.0, d1=0.0, d2=0.0)

    def check(self, got, ev, where):
        bll, b1, b2 = bounds(ev)
        ref = ev.values()
        if not np.isfinite(ref[0]):
            assert not np.isfinite(got[0]) or got[0] == ref[0], where
            return
        d = [abs(float(np.longdouble(got[i]) - x)) for i, x in enumerate((ev.ll, ev.d1, ev.d2))]
        for k, dk, bk in (("ll" if ev.n_snp >= 63 else "ll_small", d[0], bll), ("d1", d[1], b1), ("d2", d[2], b2)):
            if bk > 0:
                self.s[k] = max(self.s[k], dk / bk)
            assert dk <= bk, (where, k, dk, bk)

    def report(self, what):
        print(f"{what}: largest share of the bound: LL {self.s['ll']:.4f} where N >= 63, {self.s['ll_small']:.4f} where N < 63, "
              f"LL' {self.s['d1']:.4f}, LL'' {self.s['d2']:.4f}")


CASES = [  # seed, V, soft, rho, dense, width
    (2811, 3, False, False, False, 2),
    (2812, 8, True, True, False, 4),
    (2813, 33, False, True, False, 2),
    (2814, 65, True, False, False, 2),
    (2815, 8, True, False, True, 1),
]


@pytest.fixture(scope="module")
def solved(m):
    """Each case once: the problem, the GPU's scan (T = 2) and fit (C = 3, probe 0.5), and the restatement object."""
    out = {}
    for seed, V, soft, with_rho, dense, width in CASES:
        p = make_problem(m, seed, V, soft, dense=dense, deep=not dense)
        rho = np.where(np.arange(p["B"]) % 3 == 0, 0.0, 0.2) if with_rho else None
        anchors = np.stack([p["truth"][:, 0], p["truth"][:, 1]], axis=1).astype(np.int32)
        anchors[::11, 1] = -1
        cand = candidates(p, 3)
        e = engine_for(m, p, width)
        try:
            scan = e.share_scan(anchors, rho, p["a"] if with_rho else None)
            fit = e.share_fit(cand, rho, p["a"] if with_rho else None, probe=0.5)
            info = e.share_info()
        finally:
            e.close()
        mat, err = m["engine"].phred_tables()
        ref = R.ShareRef(p["sp"], p["g"], mat, err, p["a"] if with_rho else None, rho)
        out[seed] = dict(p=p, rho=rho, anchors=anchors, cand=cand, scan=scan, fit=fit, info=info, ref=ref)
    return out


def checked_barcodes(B):
    return list(range(min(B, len(SPECIAL)))) + list(range(len(SPECIAL), B, 5))


@pytest.mark.parametrize("seed", [c[0] for c in CASES])
def test_scan_against_the_restatement(m, solved, seed):
    s = solved[seed]
    p, ref, anchors = s["p"], s["ref"], s["anchors"]
    out, n_snp, n_read = s["scan"]
    B, V = p["B"], p["V"]
    assert out.shape == (B, 2, V, 3) and s["info"]["have_scan"] == 1 and s["info"]["n_samples"] == V and s["info"]["scan_ms"] > 0
    assert s["info"]["scan_entries"] == int((anchors >= 0).sum()) * (V - 1)
    sh = Shares()
    for b in checked_barcodes(B):
        for t in range(2):
            a = int(anchors[b, t])
            if a < 0:
                assert not out[b, t].any() and n_snp[b, t] == 0 and n_read[b, t] == 0
                continue
            assert not out[b, t, a].any()
            for v in range(V) if V <= 8 else list(range(0, V, 7)) + [V - 1]:
                if v == a:
                    continue
                sh.check(out[b, t, v], ref.evaluate(b, a, v, 0.0), (b, t, v))
            sl = slice(p["sp"].cell_pair_off[b], p["sp"].cell_pair_off[b + 1])
            ok = (ref.nrd[sl] > 0) & (p["g"][ref.snp[sl], a] != 0).any(axis=1)
            assert n_snp[b, t] == ok.sum() and n_read[b, t] == ref.nrd[sl][ok].sum()
    sh.report(f"scan, V = {V}")


@pytest.mark.parametrize("seed", [c[0] for c in CASES])
def test_fit_against_the_restated_driver(m, solved, seed):
    s = solved[seed]
    p, ref, cand, fit = s["p"], s["ref"], s["cand"], s["fit"]
    sh = Shares()
    n_case = n_near = n_star = 0
    used = cand[:, :, 0] >= 0
    assert not fit["n_eval"][~used].any() and not fit["alpha"][~used].any() and not fit["ll0"][~used].any()
    assert s["info"]["fit_used"] == used.sum() and s["info"]["fit_evals"] == fit["n_eval"][used].sum() + used.sum() and s["info"]["fit_ms"] > 0
    for b in checked_barcodes(p["B"]):
        for c in range(cand.shape[1]):
            if not used[b, c]:
                continue
            v1, v2 = (int(x) for x in cand[b, c])
            evs = {}

            def ev(a):
                if a not in evs:
                    evs[a] = ref.evaluate(b, v1, v2, a)
                return evs[a]
            near = []
            d = R.driver(lambda a: ev(a).values(), near=near)
            n_case += 1
            st, al = int(fit["status"][b, c]), float(fit["alpha"][b, c])
            e0 = ev(0.0)
            assert (fit["n_snp"][b, c], fit["n_read"][b, c]) == (e0.n_snp, e0.n_read)
            sh.check((fit["ll0"][b, c], fit["d10"][b, c], fit["d20"][b, c]), e0, (b, c, 0.0))
            sh.check((fit["ll1"][b, c], fit["d11"][b, c], fit["d21"][b, c]), ev(1.0), (b, c, 1.0))
            sh.check((fit["llp"][b, c], fit["d1p"][b, c], fit["d2p"][b, c]), ev(0.5), (b, c, 0.5))
            sh.check((fit["ll"][b, c], fit["d1"][b, c], fit["d2"][b, c]), ref.evaluate(b, v1, v2, al), (b, c, al))
            exact = e0.m1 == 0.0 and ev(1.0).m1 == 0.0           # no pair, or no term with s != 0: LL' = LL'' = +0 on both sides, no rounding
            if near and min(near) <= 1e-9 and not exact:
                n_near += 1
            else:
                assert st == d["status"] and fit["n_eval"][b, c] == d["n_eval"], (b, c, st, d["status"], fit["n_eval"][b, c], d["n_eval"])
                assert abs(al - d["alpha"]) <= 1e-9
            if st & R.INTERIOR and not st & R.NOT_CONVERGED and c < 2:
                a_star, e_star = R.maximise(ev)
                n_star += 1
                assert fit["ll"][b, c] >= float(e_star.ll) - 1e-9, (b, c, fit["ll"][b, c], float(e_star.ll))
                if -float(e_star.d2) >= 1.0:
                    assert abs(al - a_star) <= 2e-6, (b, c, al, a_star)
    print(f"fit: {n_case} cases, {n_near} left out as within 1e-9 of a branch boundary, {n_star} compared with the reference maximiser")
    assert n_near <= 0.02 * n_case and n_case >= 15
    sh.report(f"fit, V = {p['V']}")


@pytest.mark.parametrize("seed", [2812, 2814])
def test_fit_against_the_ambient_doublet_profile(m, solved, seed):
    """LL at alpha_hat, 0 and 1 from k_ambient_dbl (one serial sum per barcode, where the fit deals the pairs to 64 sums)."""
    s = solved[seed]
    p, cand, fit, ref = s["p"], s["cand"], s["fit"], s["ref"]
    rho = s["rho"] if s["rho"] is not None else np.zeros(p["B"])
    a = p["a"] if s["rho"] is not None else np.zeros(p["S"])
    e = engine_for(m, p)
    worst = 0.0
    try:
        for b in checked_barcodes(p["B"])[:12]:
            for c in range(2):
                if cand[b, c, 0] < 0 or fit["n_snp"][b, c] == 0:
                    continue
                one = np.full((p["B"], 1, 2), -1, dtype=np.int32)
                one[b, 0] = cand[b, c]
                al = float(fit["alpha"][b, c])
                shares = sorted({0.0, al, 1.0})
                ll, ns, nr = e.ambient_doublet_profile(one, shares, a, [float(rho[b])])
                assert ns[b, 0] == fit["n_snp"][b, c] and nr[b, 0] == fit["n_read"][b, c]
                ev = ref.evaluate(b, int(cand[b, c, 0]), int(cand[b, c, 1]), al)
                bound = bounds(ev)[0]
                for name, x in (("ll0", 0.0), ("ll", al), ("ll1", 1.0)):
                    d = abs(fit[name][b, c] - ll[b, 0, shares.index(x), 0])
                    if name == "ll" and bound > 0:
                        worst = max(worst, d / bound)
                    assert d <= bounds(ref.evaluate(b, int(cand[b, c, 0]), int(cand[b, c, 1]), x))[0], (b, c, name, d)
    finally:
        e.close()
    print(f"fit against k_ambient_dbl at alpha_hat: largest share of the bound {worst:.4f}")


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8).tobytes()


def sub_pileup(m, sp, cells):
    po, ro = sp.cell_pair_off, sp.cell_read_off
    pidx = np.concatenate([np.arange(po[c], po[c + 1]) for c in cells]) if len(cells) else np.zeros(0, dtype=np.int64)
    ridx = np.concatenate([np.arange(ro[c], ro[c + 1]) for c in cells]) if len(cells) else np.zeros(0, dtype=np.int64)
    npo = np.concatenate([[0], np.cumsum([po[c + 1] - po[c] for c in cells])]).astype(np.int64)
    nro = np.concatenate([[0], np.cumsum([ro[c + 1] - ro[c] for c in cells])]).astype(np.int64)
    t = np.ones(len(cells), dtype=np.int32)
    return m["synth"].SynthPileup(len(cells), sp.n_snps, npo, nro, sp.pair_snp[pidx], sp.pair_nrd[pidx], sp.reads[ridx], t, t, t, sp.truth[cells])


def test_bits(m, solved):
    s = solved[2812]
    p, rho, a, torch = s["p"], s["rho"], s["p"]["a"], m["torch"]
    B, V = p["B"], p["V"]
    anchors, cand = s["anchors"], s["cand"]
    scan0, fit0 = s["scan"][0], s["fit"]
    keys = ("alpha", "ll", "d1", "d2", "ll0", "d10", "d20", "ll1", "d11", "d21", "n_eval", "status", "n_snp", "n_read")
    e = engine_for(m, p, 2)
    try:
        e.run()
        before = (e.get_singlet(), e.get_doublet(), e.ambient_profile(p["truth"][:, 0], a, [0.0, 0.1]))
        sc = e.share_scan(anchors, rho, a)[0]
        ft = e.share_fit(cand, rho, a, probe=0.5)
        assert bits(sc) == bits(scan0) and all(bits(ft[k]) == bits(fit0[k]) for k in keys + ("llp",))       # a repeat, the other nrd_width, after run()
        after = (e.get_singlet(), e.get_doublet(), e.ambient_profile(p["truth"][:, 0], a, [0.0, 0.1]))
        for x, y in zip(before, after):
            assert all(bits(u) == bits(v) for u, v in zip(x, y))                                          # the engine's other results are as they were
        a4 = np.full((B, 4), -1, dtype=np.int32)
        a4[:, 3] = anchors[:, 0]; a4[:, 1] = anchors[:, 1]
        s4 = e.share_scan(a4, rho, a)[0]
        assert bits(s4[:, 3]) == bits(scan0[:, 0]) and bits(s4[:, 1]) == bits(scan0[:, 1]) and not s4[:, 0].any()   # T = 4, other slots
        s1 = e.share_scan(anchors[:, :1], rho, a)[0]
        assert bits(s1[:, 0]) == bits(scan0[:, 0])                                                           # T = 1
        d_anc = torch.from_numpy(anchors).to("cuda:0")
        sd = e.share_scan(int(d_anc.data_ptr()), rho, a, n_anchor=2)[0]
        assert bits(sd) == bits(scan0)                                                                       # device anchors
        c8 = np.full((B, 8, 2), -1, dtype=np.int32)
        c8[:, 7] = cand[:, 0]; c8[:, 2] = cand[:, 1]
        f8 = e.share_fit(c8, rho, a)
        f1 = e.share_fit(cand[:, :1], rho, a)
        for k in keys:
            assert bits(f8[k][:, 7]) == bits(fit0[k][:, 0]) == bits(f1[k][:, 0]), k                         # slot 0 / 7, C = 1 / 3 / 8
            assert bits(f8[k][:, 2]) == bits(fit0[k][:, 1]), k
        d_cand = torch.from_numpy(cand).to("cuda:0")
        fd = e.share_fit(int(d_cand.data_ptr()), rho, a, probe=0.5, n_cand=3)
        assert all(bits(fd[k]) == bits(fit0[k]) for k in keys + ("llp",))                                    # device cand
    finally:
        e.close()
    cells = np.array([5, 17])                               # barcodes alone: the deep pair's barcode and an ordinary one
    q = dict(p, sp=sub_pileup(m, p["sp"], cells), B=2)
    e = engine_for(m, q)
    try:
        sc = e.share_scan(anchors[cells], rho[cells], a)[0]
        ft = e.share_fit(cand[cells], rho[cells], a)
    finally:
        e.close()
    assert bits(sc) == bits(scan0[cells]) and all(bits(ft[k]) == bits(fit0[k][cells]) for k in keys)


def test_errors(m, solved):
    s = solved[2811]
    p, capi = s["p"], m["capi"]
    B, V, S = p["B"], p["V"], p["S"]
    anchors, cand, a = s["anchors"], s["cand"], p["a"]
    rho = np.full(B, 0.1)
    ARG, STATE = capi.DMX_ERR_ARG, capi.DMX_ERR_STATE

    def fails(code, f, *args, **kw):
        with pytest.raises(capi.DmxError) as ei:
            f(*args, **kw)
        assert ei.value.code == code, (ei.value.code, str(ei.value))

    e = m["engine"].Engine(V, (0.0, 0.5), 0.5)
    try:
        e.B, e.S = B, S                                                   # (the wrapper's own shape checks pass)
        fails(STATE, e.share_scan, anchors)                               # no pileup, no genotypes
        fails(STATE, e.share_fit, cand)
        e.set_genotypes(p["g"])
        e.B, e.S = B, S
        fails(STATE, e.share_scan, anchors)                               # genotypes, no pileup
        e.set_pileup(host_pileup(m, p["sp"]))
        fails(STATE, e.share_info)                                        # getters before a call
        fails(STATE, lambda: capi.check(e._L.dmx_engine_get_share_scan(e._h, None, None)))
        fails(STATE, lambda: capi.check(e._L.dmx_engine_get_share_fit(e._h, None, None)))
        fails(ARG, e.share_scan, np.zeros((B, 5), dtype=np.int32))         # T outside [1, 4]
        fails(ARG, e.share_scan, np.zeros((B, 0), dtype=np.int32))
        fails(ARG, e.share_fit, np.full((B, 9, 2), -1, dtype=np.int32))    # C outside [1, 8]
        fails(ARG, e.share_fit, np.full((B, 0, 2), -1, dtype=np.int32))
        for bad in (V, -2):
            x = anchors.copy(); x[3, 0] = bad
            fails(ARG, e.share_scan, x)                                   # an id outside [-1, V)
            y = cand.copy(); y[3, 0, 1] = bad
            fails(ARG, e.share_fit, y)
        y = cand.copy(); y[2, 1] = (1, 1)
        fails(ARG, e.share_fit, y)                                        # v1 = v2
        for r in (1.5, -0.1, np.nan):
            x = rho.copy(); x[7] = r
            fails(ARG, e.share_scan, anchors, x, a)
            fails(ARG, e.share_fit, cand, x, a)
            y = a.copy(); y[11] = r
            fails(ARG, e.share_scan, anchors, rho, y)
            fails(ARG, e.share_fit, cand, rho, y)
        fails(ARG, e.share_scan, anchors, rho, None)                      # rho without a
        fails(ARG, e.share_fit, cand, rho, None)
        for kw in (dict(tol=0.0), dict(tol=-1.0), dict(tol=np.nan), dict(max_iter=0), dict(max_iter=201), dict(start=0.0), dict(start=1.0),
                   dict(start=np.nan), dict(probe=1.5), dict(probe=np.nan)):
            fails(ARG, e.share_fit, cand, **kw)
        fails(ARG, e.share_scan, anchors, None, a[:-1])                    # n_snps
        fails(ARG, e.share_fit, cand, None, a[:-1])
        rq = capi.ShareScanRequest(B + 1, S, 2, capi.DMX_MEM_HOST, anchors.ctypes.data, None, None)
        fails(ARG, lambda: capi.check(e._L.dmx_engine_share_scan(e._h, __import__("ctypes").byref(rq))))     # n_cells
        fails(STATE, e.share_info)                                        # none of the refused calls left a result
        f = e.share_fit(cand, max_iter=1)                                 # max_iter: the one evaluation inside the bracket, then the final one
        it = (f["status"] & capi.DMX_SHARE_INTERIOR) != 0
        assert it.any() and (f["n_eval"][it] == 4).all() and ((f["status"][it] & capi.DMX_SHARE_NOT_CONVERGED) != 0).mean() > 0.9
        assert e.share_info()["have_fit"] == 1 and e.share_info()["have_scan"] == 0
        e.set_pileup(host_pileup(m, p["sp"]))
        fails(STATE, e.share_info)                                        # a new pileup drops both results
    finally:
        e.close()


def test_scan_that_cannot_fit_is_refused_before_anything_is_allocated(m):
    """V = 1 024, T = 4 and an empty pileup of so many barcodes that out[B][T][V][3] exceeds the free memory: DMX_ERR_NOMEM, the earlier scan
    of the same engine stays readable, and a small call afterwards is right.  (The fit's 120 bytes per slot cannot be made to exceed the
    device's memory with a pileup that fits the host.)"""
    capi, E = m["capi"], m["engine"]
    rng = np.random.default_rng(43)
    S, V, B = 6, 1024, 3
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = np.stack([E.geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    sp = m["synth"].make_pileup(rng, raw.alleles, B, 0.8, 2.0)
    pl = host_pileup(m, sp)
    free = m["torch"].cuda.mem_get_info(0)[0]
    nb = int(free // (4 * V * 24)) + 1024
    po = np.zeros(nb + 1, dtype=np.int64)
    zi = np.zeros(nb, dtype=np.int32)
    e = E.Engine(V, (0.0, 0.5), 0.5)
    try:
        e.set_genotypes(g); e.set_pileup(pl)
        anchors = np.array([[0], [5], [1000]], dtype=np.int32)
        first = e.share_scan(anchors)
        assert first[0].any()
        e.set_pileup(E.HostPileup(nb, S, po, po, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), zi, zi, zi))
        with pytest.raises(capi.DmxError) as ei:
            e.share_scan(np.zeros((nb, 4), dtype=np.int32))
        assert ei.value.code == capi.DMX_ERR_NOMEM
        e.set_pileup(pl)
        again = e.share_scan(anchors)
        assert all(bits(x) == bits(y) for x, y in zip(first, again))
    finally:
        e.close()


@pytest.fixture(scope="module")
def recovery(m, tmp_path_factory):
    rng = np.random.default_rng(2806)
    S, V = 4000, 8
    raw = m["synth"].make_raw_genotypes(rng, S, V)
    g = np.stack([m["engine"].geno_from_gt(raw.alleles[s], 0.01) for s in range(S)])
    kind = np.repeat([0, 1, 2], [100, 60, 60])
    alpha = np.array([0.0, 0.2, 0.1])[kind]
    sp, _, _, _ = m["synth"].make_ambient_mixed_pileup(rng, raw.alleles, len(kind), 300.0 / S, 1.0, 0.0, kind > 0, alpha)
    samples = [f"s{j}" for j in range(V)]
    barcodes = [m["synth"].barcode_name(c) for c in range(sp.n_cells)]
    prefix = str(tmp_path_factory.mktemp("share") / "rec")
    pl = host_pileup(m, sp)
    r = m["share"].share_run(pl, g, samples, prefix, barcodes=barcodes)
    return dict(r=r, sp=sp, g=g, kind=kind, alpha=alpha, samples=samples, barcodes=barcodes, prefix=prefix, pl=pl)


def test_recovery_of_unequal_doublets(m, recovery):
    """8 donors, 4 000 SNPs of which about 300 are covered by one read, 100 singlets, 60 doublets at a minor share of 0.2 and 60 at 0.1.
    The thresholds sit below what a CPU simulation of the model gave, with room for another seed; the margin of 2 is the reference's.
    Measured on the MI355X (and by the restatement on the CPU): at 0.2, 60 of 60 called DBL-, 59 with both donors right and the major one
    first, median alpha_hat 0.178; at 0.1, 54 and 47, median 0.099; no singlet called DBL-; the plain pass over {0, 0.5} calls 37 and 4 of
    the doublets DBL-: 41 of 120 against this pass's 114."""
    r, sp, kind, samples = recovery["r"], recovery["sp"], recovery["kind"], recovery["samples"]
    calls = r["calls"]
    is_dbl = np.array([c[0].startswith("DBL-") for c in calls])
    right = np.array([c[0].startswith("DBL-") and (c[1], c[2]) == (samples[sp.truth[b, 0]], samples[sp.truth[b, 1]]) for b, c in enumerate(calls)])
    al = np.array([c[3] for c in calls])
    plain = np.array([b.startswith("DBL-") for b in r["rows"].best])
    for k, share, min_dbl, min_right in ((1, 0.2, 0.9, 0.85), (2, 0.1, 0.75, 0.7)):
        sel = kind == k
        med = float(np.median(al[sel & is_dbl])) if (sel & is_dbl).any() else np.nan
        print(f"alpha = {share}: DBL- {is_dbl[sel].sum()} / 60, both donors right and the major one first {right[sel].sum()} / 60, "
              f"median alpha_hat {med:.4f}; plain pass DBL- {plain[sel].sum()} / 60")
    print(f"singlets called DBL-: {is_dbl[kind == 0].sum()} / 100 (plain pass: {plain[kind == 0].sum()}); "
          f"doublets called DBL-: {is_dbl[kind > 0].sum()} / 120 against the plain pass's {plain[kind > 0].sum()} / 120")
    for k, share, min_dbl, min_right in ((1, 0.2, 0.9, 0.85), (2, 0.1, 0.75, 0.7)):
        sel = kind == k
        assert is_dbl[sel].mean() >= min_dbl and right[sel].mean() >= min_right
        assert abs(np.median(al[sel & is_dbl]) - share) <= 0.03
    assert is_dbl[kind == 0].sum() <= 2
    assert plain[kind > 0].sum() < is_dbl[kind > 0].sum()


def test_command_line(m, recovery, tmp_path):
    """On a `demuxlet --pileup-only` style dump: without --best the plain pass's three files are written unchanged, both TSVs have the
    stated headers, and a row of each agrees with share_run's arrays; with --best nothing but the two TSVs is written, to the byte."""
    sh, refine = m["share"], m["refine"]
    sp, g, samples, barcodes, r = recovery["sp"], recovery["g"], recovery["samples"], recovery["barcodes"], recovery["r"]
    d = refine.PileupDump(samples, [(1, 100 + 10 * j, "A", "C") for j in range(sp.n_snps)], g, barcodes, recovery["pl"])
    dump = tmp_path / "x.pileup.txt"
    refine.write_pileup_txt(str(dump), d)
    assert sh.main(["--pileup", str(dump), "--out", str(tmp_path / "cl")]) == 0
    for ext in (".best", ".single", ".sing2"):
        assert (tmp_path / ("cl" + ext)).read_bytes() == open(recovery["prefix"] + ext, "rb").read()
    for ext in (".share.tsv", ".share_scan.tsv"):
        assert (tmp_path / ("cl" + ext)).read_bytes() == open(recovery["prefix"] + ext, "rb").read()
    best_bytes = (tmp_path / "cl.best").read_bytes()
    rows = [l.split("\t") for l in (tmp_path / "cl.share.tsv").read_text().splitlines()]
    assert "\t".join(rows[0]) + "\n" == sh.SHARE_HEADER and len(rows) == 1 + sp.n_cells
    k = next(i for i, c in enumerate(r["calls"]) if c[0].startswith("DBL-"))
    row = next(x for x in rows if x[0] == barcodes[k])
    c = r["calls"][k]
    assert row[1] == r["rows"].best[k] and row[2:5] == [c[0], c[1], c[2]] and row[5] == f"{c[3]:.4f}" and row[6] == f"{c[4]:.4f}"
    assert row[9] == f"{c[7]:.5f}" and row[11] == f"{c[9]:.5f}" and row[14] == str(c[12]) and row[15] == "INTERIOR" and row[16:] == [str(c[14]), str(c[15])]
    srows = [l.split("\t") for l in (tmp_path / "cl.share_scan.tsv").read_text().splitlines()]
    assert "\t".join(srows[0]) + "\n" == sh.SCAN_HEADER
    mine = [x for x in srows if x[0] == barcodes[k]]
    kept = [(t, v) for t, v in r["pick"][k] if t >= 0]
    assert len(mine) == len(kept) == 4
    t, v = kept[0]
    assert mine[0][1] == samples[r["anchors"][k, t]] and mine[0][2] == samples[v] and mine[0][4] == f"{r['scan'][k, t, v, 0]:.5f}"
    assert sh.main(["--pileup", str(dump), "--out", str(tmp_path / "b2"), "--best", str(tmp_path / "cl.best"), "--anchors", "2", "--top", "3"]) == 0
    assert not (tmp_path / "b2.best").exists() and (tmp_path / "cl.best").read_bytes() == best_bytes
    r2 = [l.split("\t") for l in (tmp_path / "b2.share.tsv").read_text().splitlines()]
    assert len(r2) == len(rows) and sum(x[2].startswith("DBL-") for x in r2[1:]) >= 0.9 * sum(x[2].startswith("DBL-") for x in rows[1:])
