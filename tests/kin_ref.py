"""Loader of tests/kin_emul.cpp (the joint-genotype-table contract of include/dmx.h as serial host code) and what
tests/test_kin_cpu.py and tests/test_gpu_kin.py share: a numpy.longdouble restatement of the table, the statistics restated with plain
loops (independent of demuxlet_amd/kin.py), the edge-row matrix, a pedigree generator, a brute-force assignment and a read simulator."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
DESCENDING, MUL_ADD = 1, 2
U = 2.0 ** -53


class KinEmu:
    def __init__(self, so):
        self.L = C.CDLL(str(so))
        for n in ("kin_set_variant", "kin_rows", "kin_table"):
            getattr(self.L, n).restype = None
        self.L.kin_set_variant.argtypes = [C.c_int]
        self.L.kin_rows.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.L.kin_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]

    def variant(self, v):
        """0 = the contract; DESCENDING or MUL_ADD = the wrong variants."""
        self.L.kin_set_variant(int(v))

    def rows(self, g, c=None):
        """(image [S][V][4] float64, valid [S][V] bool) of a matrix [S][V][3]; c [S] float64 or None."""
        g = np.ascontiguousarray(g, dtype=np.float32)
        S, V = g.shape[:2]
        img = np.zeros((S, V, 4)); valid = np.zeros((S, V), dtype=np.uint8)
        cc = None if c is None else np.ascontiguousarray(c, dtype=np.float64)
        if S * V:
            self.L.kin_rows(g.ctypes.data, S * V, V, None if cc is None else cc.ctypes.data, img.ctypes.data, valid.ctypes.data)
        return img, valid.astype(bool)

    def table(self, wa, rb):
        wa, rb = np.ascontiguousarray(wa, dtype=np.float64), np.ascontiguousarray(rb, dtype=np.float64)
        S, VA, VB = wa.shape[0], wa.shape[1], rb.shape[1]
        T = np.zeros((VA, VB, 4, 4))
        self.L.kin_table(wa.ctypes.data if S else None, rb.ctypes.data if S else None, S, VA, VB, T.ctypes.data)
        return T

    def compare(self, ga, gb=None, c=None):
        """(T, n_valid_a, n_valid_b) of the whole contract."""
        wa, va = self.rows(ga, c)
        rb, vb = self.rows(ga if gb is None else gb, None)
        return self.table(wa, rb), va.sum(axis=0).astype(np.int32), vb.sum(axis=0).astype(np.int32)


def build(out_dir):
    so = Path(out_dir) / "libkin_emul.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(ROOT / "tests" / "kin_emul.cpp"), "-o", str(so), "-lm"])
    return KinEmu(so)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def table_longdouble(wa, rb):
    """The table from the emulator's own rounded wa / rb in numpy.longdouble, SNP by SNP."""
    wa, rb = np.asarray(wa).astype(np.longdouble), np.asarray(rb).astype(np.longdouble)
    T = np.zeros((wa.shape[1], rb.shape[1], 4, 4), dtype=np.longdouble)
    for i in range(wa.shape[0]):
        T += wa[i][:, None, :, None] * rb[i][None, :, None, :]
    return T


def chain_bound(S, T):
    """S u / (1 - S u) T: the standard bound for a chain of S roundings over non-negative terms."""
    return (S * U / (1.0 - S * U)) * np.asarray(T, dtype=np.longdouble)


# ---------------------------------------------------------------------------------------------------------------------
# inputs

SPECIAL_ROWS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0.5, 0.5, 0), (0, 0.25, 0.75), (0.5, 0, 0.5), (0.3, -0.1, 0.8), (np.nan, 0.5, 0.5),
                (1e-45, 1e-45, 1e-45), (1e-45, 0, 1e-45), (0, 1e-45, 0), (np.inf, 0, 0), (2.0, 3.0, 5.0)]
SPECIAL_VALID = [False, True, True, True, True, True, True, False, False, True, True, True, False, True]


def edge_matrix(rng, S, V):
    """Soft rows with tests/test_gpu_redraw.py's edge_matrix kinds of rows scattered over them (as many as fit): all zero, hard zeros in
    every position, a negative entry, NaN, inf, float32 subnormals, an unnormalised row (2, 3, 5)."""
    g = rng.dirichlet(np.ones(3), size=(S, V)).astype(np.float32)
    cells = rng.permutation(S * V)[:3 * len(SPECIAL_ROWS)]
    for k, t in enumerate(cells):
        g[t // V, t % V] = np.array(SPECIAL_ROWS[k % len(SPECIAL_ROWS)], dtype=np.float32)
    return g


def edge_weight(rng, S):
    """Random weights with zeros and one subnormal."""
    c = rng.uniform(0.0, 3.0, size=S)
    c[rng.random(S) < 0.2] = 0.0
    if S:
        c[rng.integers(0, S)] = 5e-324
    return c


PEDIGREE = ["A", "B", "C", "D", "k1", "k2", "h", "dup"]
REL1_PAIRS = {("A", "k1"), ("A", "k2"), ("B", "k1"), ("B", "k2"), ("A", "h"), ("C", "h"), ("A", "dup"), ("B", "dup"), ("k1", "k2"), ("k2", "dup")}
REL2_PAIRS = {("k1", "h"), ("k2", "h"), ("h", "dup")}
DUP_PAIRS = {("k1", "dup")}


def expected_band(a, b):
    """"DUP", "REL1", "REL2" or "." for two names of PEDIGREE."""
    for name, s in (("DUP", DUP_PAIRS), ("REL1", REL1_PAIRS), ("REL2", REL2_PAIRS)):
        if (a, b) in s or (b, a) in s:
            return name
    return "."


def pedigree(rng, S):
    """Hard one-hot float32 rows [S][8][3] of PEDIGREE over unlinked SNPs with allele frequencies uniform in [0.05, 0.5]: founders A, B, C
    and D, k1 and k2 children of A and B, h a child of A and C (a half-sibling of k1 and k2), dup a copy of k1."""
    f = rng.uniform(0.05, 0.5, size=S)
    hap = {n: (rng.random((S, 2)) < f[:, None]).astype(np.int64) for n in "ABCD"}

    def child(p, q):
        i = np.arange(S)
        return np.stack([hap[p][i, rng.integers(0, 2, size=S)], hap[q][i, rng.integers(0, 2, size=S)]], axis=1)

    hap["k1"], hap["k2"], hap["h"] = child("A", "B"), child("A", "B"), child("A", "C")
    hap["dup"] = hap["k1"]
    g = np.zeros((S, len(PEDIGREE), 3), dtype=np.float32)
    for j, n in enumerate(PEDIGREE):
        g[np.arange(S), j, hap[n].sum(axis=1)] = 1.0
    return g


# ---------------------------------------------------------------------------------------------------------------------
# the statistics, with plain loops

def ref_stats(t):
    """dict(N, IBS0, IBS2, DISC, R, KIN) of one 4 x 4 table."""
    J = [[float(t[x][y]) for y in range(3)] for x in range(3)]
    N = float(t[3][3])
    tot = sum(sum(r) for r in J)
    ibs0 = (J[0][2] + J[2][0]) / N
    ibs2 = (J[0][0] + J[1][1] + J[2][2]) / N
    row = [sum(J[x]) for x in range(3)]
    col = [sum(J[x][y] for x in range(3)) for y in range(3)]
    ea = sum(x * row[x] for x in range(3)) / tot
    eb = sum(y * col[y] for y in range(3)) / tot
    va = sum(x * x * row[x] for x in range(3)) / tot - ea * ea
    vb = sum(y * y * col[y] for y in range(3)) / tot - eb * eb
    eab = sum(x * y * J[x][y] for x in range(3) for y in range(3)) / tot
    r = (eab - ea * eb) / (va * vb) ** 0.5 if va > 0 and vb > 0 else float("nan")
    den = row[1] + col[1]
    kin = (J[1][1] - 2.0 * (J[0][2] + J[2][0])) / den if den > 0 else float("nan")
    return dict(N=N, IBS0=ibs0, IBS2=ibs2, DISC=1.0 - ibs2, R=r, KIN=kin)


def ref_read_model(mat, err):
    """By base quality: L[q][g][al] (the singlet pass's read likelihood under genotype g) and P[q][g][al] (the law of a stored read)."""
    L = np.zeros((128, 3, 2)); P = np.zeros((128, 3, 2))
    for q in range(128):
        m, e3 = float(mat[q]), float(err[q]) / 3.0
        L[q, 0] = (m, e3); L[q, 1] = ((m + e3) / 2, (m + e3) / 2); L[q, 2] = (e3, m)
        for g_ in range(3):
            P[q, g_] = L[q, g_] / (L[q, g_, 0] + L[q, g_, 1])
    return L, P


def ref_gl(L, q, al):
    """The singlet pass's genotype likelihoods of one pair from its reads (q[n], al[n]): the running product normalised after every
    read, then + 1e-6 and normalised again (cmd_cram_demuxlet.cpp:427-452)."""
    gl = np.ones(3)
    for qq, a in zip(q, al):
        gl = gl * L[qq, :, a]
        gl = gl / gl.sum()
    gl = gl + 1e-6
    return gl / gl.sum()


def ref_kl(mat, err, bq_weights):
    """KL[x][y] = sum_q w_q sum_al P[q][x][al] (log GL_x - log GL_y) of a pair with the one read (q, al)."""
    L, P = ref_read_model(mat, err)
    w = np.asarray(bq_weights, dtype=np.float64) / np.sum(bq_weights)
    kl = np.zeros((3, 3))
    for q in np.nonzero(w)[0]:
        for al in range(2):
            lg = np.log(ref_gl(L, [q], [al]))
            for x in range(3):
                for y in range(3):
                    kl[x, y] += w[q] * P[q, x, al] * (lg[x] - lg[y])
    return kl


def simulate_llr(rng, xa, xb, c, mat, err, bqs, n_cells):
    """llk_a - llk_b, as the singlet pass computes them for hard rows, of n_cells cells of a donor with the genotypes xa [S], against
    xb [S]: Poisson(c_i) reads per SNP, base qualities uniform over bqs, alleles from the law of a stored read."""
    L, P = ref_read_model(mat, err)
    out = np.zeros(n_cells)
    for k in range(n_cells):
        n = rng.poisson(c)
        for i in np.nonzero(n)[0]:
            q = np.asarray(bqs)[rng.integers(0, len(bqs), size=n[i])]
            al = (rng.random(n[i]) < P[q, xa[i], 1]).astype(np.int64)
            lg = np.log(ref_gl(L, q, al))
            out[k] += lg[xa[i]] - lg[xb[i]]
    return out


def brute_assign(gain, allowed=None):
    """The best total of a one-to-one partial assignment over allowed pairs with gain > 0: every row tries every free column and
    'unassigned', exhaustively."""
    gain = np.asarray(gain, dtype=np.float64)
    nA, nB = gain.shape
    ok = gain > 0 if allowed is None else (gain > 0) & np.asarray(allowed, dtype=bool)

    def rec(i, used):
        if i == nA:
            return 0.0
        best = rec(i + 1, used)
        for j in range(nB):
            if ok[i, j] and j not in used:
                best = max(best, gain[i, j] + rec(i + 1, used | {j}))
        return best

    return rec(0, frozenset())


def match_problem(rng, S=3000, V=6):
    """A: V unrelated hard columns over S SNPs.  B: the same donors in a permuted order plus one more unrelated donor, 2 % of its
    genotypes changed to another one and 30 % of its (SNP, column) rows not covered.  Returns (ga [S][V][3], gb [S][V + 1][3] hard rows,
    covered [S][V + 1] bool, perm) with B's column perm[a] holding A's column a; B's last donor can be anywhere but at perm[.]."""
    f = rng.uniform(0.05, 0.5, size=S)
    x = (rng.random((S, V + 1, 2)) < f[:, None, None]).sum(axis=2)          # genotypes of V + 1 unrelated donors
    order = rng.permutation(V + 1)                                          # B's column j holds donor order[j]
    xb = x[:, order].copy()
    flip = rng.random(xb.shape) < 0.02
    xb[flip] = (xb[flip] + rng.integers(1, 3, size=int(flip.sum()))) % 3
    covered = rng.random(xb.shape) >= 0.30
    eye = np.eye(3, dtype=np.float32)
    perm = np.array([int(np.nonzero(order == a)[0][0]) for a in range(V)])
    return eye[x[:, :V]], eye[xb], covered, perm
