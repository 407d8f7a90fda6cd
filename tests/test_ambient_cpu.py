"""CPU: the host side of the ambient contamination profile (demuxlet_amd/ambient.py) — argument checks, the summary rules, the ambient
frequency builders, the TSV writers, the command line's argument errors — and the numpy restatement (tests/ambient_ref.py) against a
brute-force per-read product.  No GPU compute is called."""
import numpy as np
import pytest

import ambient_ref as R


@pytest.fixture(scope="module")
def mods():
    from demuxlet_amd import ambient, build, capi, engine, synth
    build.build()
    capi.load()
    return dict(ambient=ambient, capi=capi, engine=engine, synth=synth)


def test_default_grid(mods):
    A = mods["ambient"]
    g = A.default_grid()
    assert len(g) == 51 and g[0] == 0.0 and g[-1] == 0.5 and np.all(np.diff(g) > 0)
    assert np.allclose(g, np.arange(51) * 0.01, atol=1e-15)
    assert len(A.default_grid(1.0, 0.25)) == 5
    with pytest.raises(ValueError):
        A.default_grid(0.5, 0.0)
    with pytest.raises(ValueError):
        A.default_grid(0.5, 0.001)               # 501 points


@pytest.mark.parametrize("grid", [[], [0.2, 0.1], [0.1, 0.1], [-0.01, 0.2], [0.5, 1.01], [0.0, float("nan")], list(np.linspace(0, 1, 257))])
def test_bad_grids(mods, grid):
    with pytest.raises(ValueError):
        mods["ambient"].check_grid(grid)


def test_good_grids(mods):
    A = mods["ambient"]
    assert len(A.check_grid([0.3])) == 1
    assert len(A.check_grid(np.linspace(0, 1, 256))) == 256


def test_ambient_and_assign_checks(mods):
    A = mods["ambient"]
    assert A.check_ambient([0.0, 0.5, 1.0], 3).dtype == np.float64
    for bad in ([0.0, 1.5, 0.2], [-1e-9, 0.1, 0.2], [0.1, float("nan"), 0.2]):
        with pytest.raises(ValueError):
            A.check_ambient(bad, 3)
    with pytest.raises(ValueError):
        A.check_ambient([0.1, 0.2], 3)
    assert A.check_assign([-1, 0, 2], 3, 3).tolist() == [-1, 0, 2]
    with pytest.raises(ValueError):
        A.check_assign([0, 1], 3, 3)             # length
    with pytest.raises(ValueError):
        A.check_assign([0, 3, -1], 3, 3)         # sample out of range
    with pytest.raises(ValueError):
        A.check_assign([0, -2, -1], 3, 3)


def test_summary_rules(mods):
    A = mods["ambient"]
    grid = np.array([0.0, 0.1, 0.2, 0.3, 0.4])
    ll = np.array([
        [-10.0, -8.0, -5.0, -6.0, -9.0],         # argmax 0.2; within 1.92: 0.2, 0.3 (-6.0 >= -6.92); -8.0 is not
        [-3.0, -3.0, -4.0, -7.0, -8.0],          # tie at the top: the lowest index; interval [0.0, 0.2] (-4.0 >= -4.92)
        [-1.0, -2.92, -2.93, -2.0, -5.0],        # -2.92 is exactly max - 1.92: inside; the interval spans 0.0 .. 0.3 (largest point inside)
        [-5.0, -5.0, -5.0, -5.0, -5.0],          # flat: rho 0, interval the whole grid
    ])
    s = A.summarize(ll, grid)
    assert s.rho.tolist() == [0.2, 0.0, 0.0, 0.0]
    assert s.rho_lo.tolist() == [0.2, 0.0, 0.0, 0.0]
    assert s.rho_hi.tolist() == [0.3, 0.2, 0.3, 0.4]
    assert s.llk_rho.tolist() == [-5.0, -3.0, -1.0, -5.0]
    assert s.llk_0.tolist() == [-10.0, -3.0, -1.0, -5.0]
    assert s.llr.tolist() == [5.0, 0.0, 0.0, 0.0]
    s2 = A.summarize(ll[:, 1:], grid[1:])      # no 0 in the grid: LLK.0 and LLR are NaN
    assert np.isnan(s2.llk_0).all() and np.isnan(s2.llr).all()
    with pytest.raises(ValueError):
        A.summarize(ll, grid[:4])


def test_pool_profile_is_a_serial_sum(mods):
    A = mods["ambient"]
    rng = np.random.default_rng(5)
    ll = rng.normal(-100.0, 30.0, size=(200, 7))
    assign = rng.integers(-1, 3, size=200)
    want = np.zeros(7)
    for b in range(200):
        if assign[b] >= 0:
            want = want + ll[b]
    got = A.pool_profile(ll, assign)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert not A.pool_profile(ll, np.full(200, -1)).any()


def test_ambient_builders(mods):
    A = mods["ambient"]
    assert np.allclose(A.ambient_from_counts([0, 8, 3], [0, 2, 3]), [0.5, 0.25, 0.5])
    g = np.zeros((2, 3, 3), dtype=np.float32)
    g[0, :, :] = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]            # SNP 0: dosages 0, 1, 2
    g[1, :, :] = [[0, 0, 1], [0.5, 0.5, 0], [0.2, 0.2, 0.6]]
    assign = np.array([0, 0, 1, 2, -1, 2, 2, 2])               # pi = (2, 1, 4) / 7
    pi = np.array([2, 1, 4]) / 7.0
    want0 = pi @ np.array([0.0, 0.5, 1.0])
    want1 = pi @ np.array([1.0, 0.25, 0.1 + 0.6])
    a = A.ambient_from_genotypes(g, assign)
    assert np.allclose(a, [want0, want1], atol=1e-7)
    with pytest.raises(ValueError):
        A.ambient_from_genotypes(g, np.full(4, -1))


def test_writers(mods, tmp_path):
    A = mods["ambient"]
    grid = np.array([0.0, 0.05, 0.1])
    ll = np.array([[-10.0, -9.0, -9.5], [0.0, 0.0, 0.0], [-3.0, -4.0, -6.0]])
    assign = np.array([1, -1, 0])
    s = A.summarize(ll, grid)
    A.write_ambient_tsv(str(tmp_path / "x.ambient.tsv"), ["AAA-1", "CCC-1", "GGG-1"], ["S0", "S1"], assign, [10, 0, 7], [12, 0, 9], s)
    lines = (tmp_path / "x.ambient.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["BARCODE", "SM_ID", "N.SNP", "N.READ", "RHO", "RHO.LO", "RHO.HI", "LLK.RHO", "LLK.0", "LLR"]
    assert len(lines) == 3
    assert lines[1].split("\t") == ["AAA-1", "S1", "10", "12", "0.0500", "0.0000", "0.1000", "-9.00000", "-10.00000", "1.00000"]
    assert lines[2].split("\t")[:5] == ["GGG-1", "S0", "7", "9", "0.0000"]
    pool = A.pool_profile(ll, assign)
    est = A.write_pool_tsv(str(tmp_path / "x.ambient_pool.tsv"), grid, pool)
    assert est == 0.0
    p = (tmp_path / "x.ambient_pool.tsv").read_text().splitlines()
    assert p[0] == "RHO\tLLK" and len(p) == 5
    assert p[2] == "0.0500\t-13.00000" and p[-1] == "#RHO.POOL\t0.0000"


def test_cli_argument_errors(mods):
    A = mods["ambient"]
    base = ["--pileup", "x.pileup.txt", "--out", "o"]
    a = A.parse_args(base)
    assert len(a.grid) == 51 and a.ambient == "reads" and a.best is None
    assert A.parse_args(base + ["--grid", "0", "0.2", "0.4"]).grid.tolist() == [0.0, 0.2, 0.4]
    assert len(A.parse_args(base + ["--grid-max", "0.3", "--grid-step", "0.1"]).grid) == 4
    for extra in (["--grid", "0.3", "0.2"], ["--grid", "1.5"], ["--grid-step", "0"], ["--grid-max", "2"], ["--ambient", "empty"],
                  ["--min-prb", "1.5"], ["--grid-step", "0.001"]):
        with pytest.raises(SystemExit):
            A.parse_args(base + extra)
    with pytest.raises(SystemExit):
        A.parse_args(["--out", "o"])


def test_synthetic_ambient_pileup(mods):
    synth = mods["synth"]
    rng = np.random.default_rng(3)
    raw = synth.make_raw_genotypes(rng, 400, 4)
    rho = np.array([0.0, 0.3] * 10)
    sp, r, a = synth.make_ambient_pileup(rng, raw.alleles, 20, 0.5, 1.5, rho)
    assert np.array_equal(r, rho) and a.shape == (400,)
    assert np.allclose(a, np.clip(raw.alleles, 0, 1).sum(axis=2).mean(axis=1) / 2)
    assert sp.cell_read_off[-1] == len(sp.reads) == int(sp.pair_nrd.sum())
    assert (sp.truth[:, 1] == -1).all() and sp.truth[:, 0].tolist() == [c % 4 for c in range(20)]
    dense, _, _ = synth.make_ambient_pileup(rng, raw.alleles, 5, 1.0, 1.2, 0.1, dense_layout=True)
    assert dense.pair_snp is None and dense.cell_pair_off[-1] == 5 * 400


def brute_profile(pairs, g, a, grid, mat, err):
    """Per barcode, the per-read product in mpmath at 200 bits, then the log: no rescaling needed, no underflow possible."""
    import mpmath
    out = []
    with mpmath.workprec(200):
        _brute(pairs, g, a, grid, mat, err, out, mpmath)
    return np.array(out)


def _brute(pairs, g, a, grid, mat, err, out, mpmath):
    for rho in grid:
        tot = mpmath.mpf(0)
        for snp, rd in pairs:
            f = [mpmath.mpf(1)] * 3
            for b in rd:
                bq, alt = b & 127, b >> 7
                pR = mpmath.mpf(err[bq]) / 3 if alt else mpmath.mpf(mat[bq])
                pA = mpmath.mpf(mat[bq]) if alt else mpmath.mpf(err[bq]) / 3
                for gg in range(3):
                    p = (1 - mpmath.mpf(rho)) * gg / 2 + mpmath.mpf(rho) * mpmath.mpf(a[snp])
                    f[gg] *= pR * (1 - p) + pA * p
            L = sum(mpmath.mpf(float(g[snp][gg])) * f[gg] for gg in range(3))
            tot += mpmath.log(L)
        out.append(float(tot))


def test_restatement_against_brute_force(mods):
    """One barcode of a few pairs (a REF read, an ALT read, mixed pairs, a gp row with hard zeros, an all-zero row and a pair without
    reads that do not count), then a pair of 400 high-quality mismatching reads whose plain float64 product underflows to 0."""
    mat, err = mods["engine"].phred_tables()
    g = np.array([[0.98, 0.01, 0.01], [0.2, 0.5, 0.3], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.6, 0.4, 0.0], [0.3, 0.3, 0.4], [1.0, 0.0, 0.0]],
                 dtype=np.float32)
    a = np.array([0.3, 0.0, 1.0, 0.5, 0.7, 0.5, 0.5])
    grid = np.array([0.0, 0.05, 0.5, 1.0])
    byte = lambda alt, bq: (alt << 7) | bq
    pairs = [(0, [byte(0, 30)]), (1, [byte(1, 20), byte(0, 35), byte(1, 13)]), (2, [byte(0, 40), byte(0, 25)]), (3, [byte(1, 30)]),
             (4, [byte(1, 38)] * 5), (5, [])]
    po = np.array([0, len(pairs)])
    snp = np.array([s for s, _ in pairs])
    nrd = np.array([len(r) for _, r in pairs])
    reads = np.array([b for _, r in pairs for b in r], dtype=np.uint8)
    ll, n_snp, n_read = R.ref_profile(po, snp, nrd, reads, np.array([0]), g[:, None, :], a, grid, mat, err)
    counted = [pairs[k] for k in (0, 1, 2, 4)]              # SNP 3: all-zero gp row; SNP 5: no stored read
    want = brute_profile(counted, g, a, grid, mat, err)
    assert np.abs(ll[0] - want).max() < 1e-12
    assert n_snp.tolist() == [4] and n_read.tolist() == [11]

    deep = [(6, [byte(1, 40)] * 400)]                         # hom REF, 400 ALT reads at bq 40: (1e-4 / 3)^400 ~ 1e-1800
    d_reads = np.array(deep[0][1], dtype=np.uint8)
    ll2, _, _ = R.ref_profile(np.array([0, 1]), np.array([6]), np.array([400]), d_reads, np.array([0]), g[:, None, :], a, grid, mat, err)
    want2 = brute_profile(deep, g, a, grid, mat, err)
    assert np.abs(ll2[0] - want2).max() < 1e-9 * max(1.0, np.abs(want2).max() / 1e4)
    naive = 1.0
    for _ in range(400):
        naive *= err[40] / 3.0                                # what a product without rescaling computes at rho = 0
    assert naive == 0.0 and np.isfinite(ll2[0, 0]) and ll2[0, 0] < -4000
