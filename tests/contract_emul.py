"""Loader of tests/contract_emul.cpp (the feature passes' contracts of include/dmx.h as serial host code) and the inputs that
tests/test_contract_emul_cpu.py and tests/test_gpu_contract_bits.py share.

build(dir) compiles the emulator the way tests/test_dmx_log.py compiles log_emul.cpp and loads it with ctypes; build(dir, contract=True)
is the same source with -ffp-contract=fast (one of the three wrong variants; the other two are Emulator.variant).

The inputs: pileups of tests/quality_mix.mixed_depth_pileup cut to exact pair counts per barcode (0, 1, 63, 64, 65, 129: the kernels'
trip of 64 pair headers, its tail and a second trip), dense ones of exactly those SNP counts, read counts as u8 / u16 / u32, genotype
matrices with all-zero rows, hard zeros and a row of float32 subnormals, and hand-built pairs where a count or a path must be exact."""
import ctypes as C
import subprocess
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Tuple

import numpy as np

import quality_mix as QM

ROOT = Path(__file__).resolve().parents[1]
DESCENDING, LIBM_LOG = 1, 2
PAIR_COUNTS = (0, 1, 63, 64, 65, 129)


class EmuPileup(C.Structure):
    _fields_ = [("n_cells", C.c_int32), ("n_snps", C.c_int32), ("cell_pair_off", C.c_void_p), ("cell_read_off", C.c_void_p),
                ("pair_snp", C.c_void_p), ("pair_nrd", C.c_void_p), ("nrd_width", C.c_int32), ("reserved", C.c_int32), ("reads", C.c_void_p)]


def _f64(x): return np.ascontiguousarray(x, dtype=np.float64)
def _i32(x): return np.ascontiguousarray(x, dtype=np.int32)


class Emulator:
    def __init__(self, so):
        self.L = C.CDLL(str(so))
        for name in ("emu_set_variant", "emu_log_n", "emu_ambient", "emu_ambient_doublet", "emu_fit", "emu_refine", "emu_cluster_stage",
                     "emu_cluster_mstep"):
            getattr(self.L, name).restype = None
        self.L.emu_set_variant.argtypes = [C.c_int]
        self.L.emu_log_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        P, V, I = C.POINTER(EmuPileup), C.c_void_p, C.c_int32
        self.L.emu_ambient.argtypes = [P, V, I, V, V, V, V, V, I, V, V, V, V]
        self.L.emu_ambient_doublet.argtypes = [P, V, I, V, V, V, I, V, I, V, V, I, V, V, V, V]
        self.L.emu_fit.argtypes = [P, V, I, V, V, V, V, V, V, I, V, V, V, V, V, V, V, V]
        self.L.emu_refine.argtypes = [P, I, I, V, V, V, V, V, V, V, V]
        self.L.emu_cluster_stage.argtypes = [P, V, V, V, V, V, V, V]
        self.L.emu_cluster_mstep.argtypes = [I, I, V, V, V, V, V, V]

    def variant(self, v):
        """0 = the contract; DESCENDING and / or LIBM_LOG = the wrong variants."""
        self.L.emu_set_variant(int(v))

    def log(self, x):
        x = _f64(x)
        y = np.zeros_like(x)
        self.L.emu_log_n(x.ctypes.data, y.ctypes.data, x.size)
        return y

    @staticmethod
    def _pileup(sp):
        keep = dict(po=np.ascontiguousarray(sp.cell_pair_off, dtype=np.int64), ro=np.ascontiguousarray(sp.cell_read_off, dtype=np.int64),
                    snp=None if sp.pair_snp is None else _i32(sp.pair_snp), nrd=np.ascontiguousarray(sp.pair_nrd),
                    rd=np.ascontiguousarray(sp.reads, dtype=np.uint8))
        assert keep["nrd"].dtype in (np.uint8, np.uint16, np.uint32)
        st = EmuPileup(sp.n_cells, sp.n_snps, keep["po"].ctypes.data, keep["ro"].ctypes.data,
                       None if keep["snp"] is None else keep["snp"].ctypes.data, keep["nrd"].ctypes.data, keep["nrd"].dtype.itemsize, 0,
                       keep["rd"].ctypes.data)
        return st, keep

    @staticmethod
    def _counters(c):
        return dict(log_zero=int(c[0]), log_other=int(c[1]), rescales=int(c[2]))

    def ambient(self, sp, g, mat, err, assign, ambient, grid):
        """(ll[B][Q], n_snp[B], n_read[B], counters) of dmx_engine_ambient's contract."""
        st, keep = self._pileup(sp)
        g = np.ascontiguousarray(g, dtype=np.float32); mat, err = _f64(mat), _f64(err)
        assign, amb, grid = _i32(assign), _f64(ambient), _f64(grid)
        B, Q = sp.n_cells, len(grid)
        ll = np.zeros((B, Q)); n_snp = np.zeros(B, dtype=np.int32); n_read = np.zeros(B, dtype=np.int32); cnt = np.zeros(3, dtype=np.int64)
        self.L.emu_ambient(C.byref(st), g.ctypes.data, g.shape[1], mat.ctypes.data, err.ctypes.data, assign.ctypes.data, amb.ctypes.data,
                           grid.ctypes.data, Q, ll.ctypes.data, n_snp.ctypes.data, n_read.ctypes.data, cnt.ctypes.data)
        return ll, n_snp, n_read, self._counters(cnt)

    def ambient_doublet(self, sp, g, mat, err, cand, alphas, ambient, grid):
        """(ll[B][C][A][Q], n_snp[B][C], n_read[B][C], counters) of dmx_engine_ambient_doublet's contract."""
        st, keep = self._pileup(sp)
        g = np.ascontiguousarray(g, dtype=np.float32); mat, err = _f64(mat), _f64(err)
        cand, al, amb, grid = _i32(cand), _f64(alphas), _f64(ambient), _f64(grid)
        B, Cn, A, Q = sp.n_cells, cand.shape[1], len(al), len(grid)
        ll = np.zeros((B, Cn, A, Q)); n_snp = np.zeros((B, Cn), dtype=np.int32); n_read = np.zeros((B, Cn), dtype=np.int32)
        cnt = np.zeros(3, dtype=np.int64)
        self.L.emu_ambient_doublet(C.byref(st), g.ctypes.data, g.shape[1], mat.ctypes.data, err.ctypes.data, cand.ctypes.data, Cn,
                                   al.ctypes.data, A, amb.ctypes.data, grid.ctypes.data, Q, ll.ctypes.data, n_snp.ctypes.data,
                                   n_read.ctypes.data, cnt.ctypes.data)
        return ll, n_snp, n_read, self._counters(cnt)

    def fit(self, sp, g, mat, err, hyp, alpha, rho, ambient, M):
        """(dict of obs / mean / var / n_snp / n_read / n_trunc / n_zero [B], counters) of dmx_engine_fit's contract."""
        st, keep = self._pileup(sp)
        g = np.ascontiguousarray(g, dtype=np.float32); mat, err = _f64(mat), _f64(err)
        hyp, al = _i32(hyp), _f64(alpha)
        rh = None if rho is None else _f64(rho)
        amb = None if ambient is None else _f64(ambient)
        B = sp.n_cells
        out = {k: np.zeros(B) for k in ("obs", "mean", "var")}
        out.update({k: np.zeros(B, dtype=np.int32) for k in ("n_snp", "n_read", "n_trunc", "n_zero")})
        cnt = np.zeros(3, dtype=np.int64)
        self.L.emu_fit(C.byref(st), g.ctypes.data, g.shape[1], mat.ctypes.data, err.ctypes.data, hyp.ctypes.data, al.ctypes.data,
                       None if rh is None else rh.ctypes.data, None if amb is None else amb.ctypes.data, int(M),
                       *(out[k].ctypes.data for k in ("obs", "mean", "var", "n_snp", "n_read", "n_trunc", "n_zero")), cnt.ctypes.data)
        return out, self._counters(cnt)

    def refine(self, sp, S, V, mat, err, assign):
        """(ll[S][V][3], n_cell, n_ref, n_alt [S][V], counters) of dmx_engine_refine_genotypes' contract."""
        st, keep = self._pileup(sp)
        mat, err, assign = _f64(mat), _f64(err), _i32(assign)
        ll = np.zeros((S, V, 3)); n_cell, n_ref, n_alt = (np.zeros((S, V), dtype=np.int32) for _ in range(3)); cnt = np.zeros(3, dtype=np.int64)
        self.L.emu_refine(C.byref(st), S, V, mat.ctypes.data, err.ctypes.data, assign.ctypes.data, ll.ctypes.data, n_cell.ctypes.data,
                          n_ref.ctypes.data, n_alt.ctypes.data, cnt.ctypes.data)
        return ll, n_cell, n_ref, n_alt, self._counters(cnt)

    def cluster_stage(self, sp, mat, err):
        """(snp_off[S + 1] i64, cell[P] i32, lgl[P][3] f64, ref_alt[P] u32, counters) of dmx_engine_cluster_stage's contract."""
        st, keep = self._pileup(sp)
        mat, err = _f64(mat), _f64(err)
        P = len(keep["nrd"])
        off = np.zeros(sp.n_snps + 1, dtype=np.int64); cell = np.zeros(P, dtype=np.int32); lgl = np.zeros((P, 3))
        ra = np.zeros(P, dtype=np.uint32); cnt = np.zeros(3, dtype=np.int64)
        self.L.emu_cluster_stage(C.byref(st), mat.ctypes.data, err.ctypes.data, off.ctypes.data, cell.ctypes.data, lgl.ctypes.data,
                                 ra.ctypes.data, cnt.ctypes.data)
        return off, cell, lgl, ra, self._counters(cnt)

    def cluster_mstep(self, off, cell, lgl, w):
        """(LL[S][C][3], W[S][C]) of dmx_engine_cluster_mstep's contract over a stage cache."""
        off = np.ascontiguousarray(off, dtype=np.int64); cell = _i32(cell); lgl = _f64(lgl); w = _f64(w)
        S, Cn = len(off) - 1, w.shape[1]
        LL = np.zeros((S, Cn, 3)); W = np.zeros((S, Cn))
        self.L.emu_cluster_mstep(S, Cn, off.ctypes.data, cell.ctypes.data, lgl.ctypes.data, w.ctypes.data, LL.ctypes.data, W.ctypes.data)
        return LL, W


def build(out_dir, contract=False):
    """The emulator built into out_dir.  contract=True: the wrong variant whose products contract into FMAs (-mfma, so that g++ has an
    instruction to contract into; EMU_FUSE_SHARED_PRODUCTS, so that the genotype-likelihood recurrence, whose products g++ leaves alone
    because each is also used on its own, is contracted as a device compiler would)."""
    so = Path(out_dir) / ("libcontract_emul_fast.so" if contract else "libcontract_emul.so")
    flags = ["-ffp-contract=fast", "-mfma", "-DEMU_FUSE_SHARED_PRODUCTS"] if contract else ["-ffp-contract=off"]
    subprocess.check_call(["g++", "-O2", *flags, "-shared", "-fPIC", f"-I{ROOT / 'demuxlet_amd' / 'csrc'}",
                           str(ROOT / "tests" / "contract_emul.cpp"), "-o", str(so), "-lm"])
    return Emulator(so)


def bits(x):
    """The unsigned-integer view that the bit comparisons use."""
    x = np.ascontiguousarray(x)
    return x.view({8: np.uint64, 4: np.uint32}[x.dtype.itemsize])


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------

@dataclass
class Problem:
    name: str
    sp: object                      # a synth.SynthPileup
    g: np.ndarray                   # float32 [S][V][3]
    tables: Optional[Tuple[np.ndarray, np.ndarray]] = None       # the engine's own phred tables when None
    deep: bool = False              # holds pairs of >= 8 reads that the ambient passes must rescale

    @property
    def V(self): return self.g.shape[1]


def filter_pairs(synth, sp, keep):
    """The pileup without the pairs whose keep[] is false, as a sparse one (a dense pileup's pair t of a barcode is SNP t)."""
    B, S = sp.n_cells, sp.n_snps
    po = np.asarray(sp.cell_pair_off, dtype=np.int64)
    cell = np.repeat(np.arange(B), np.diff(po))
    snp = np.asarray(sp.pair_snp) if sp.pair_snp is not None else np.arange(len(cell)) - po[cell]
    nrd = np.asarray(sp.pair_nrd).astype(np.int64)
    start = np.cumsum(nrd) - nrd
    idx = np.flatnonzero(keep)
    new_po = np.concatenate([[0], np.cumsum(np.bincount(cell[idx], minlength=B))]).astype(np.int64)
    new_ro = np.concatenate([[0], np.cumsum(np.bincount(cell[idx], weights=nrd[idx], minlength=B))]).astype(np.int64)
    rd = np.asarray(sp.reads)
    reads = np.concatenate([rd[start[i]:start[i] + nrd[i]] for i in idx] + [np.zeros(0, dtype=np.uint8)]).astype(np.uint8)
    nr = nrd[idx]
    t = np.diff(new_ro).astype(np.int32)
    return synth.SynthPileup(B, S, new_po, new_ro, snp[idx].astype(np.int32), nr.astype(np.uint8 if nr.max(initial=0) <= 255 else np.uint16),
                             reads, t, t.copy(), t.copy(), sp.truth.copy())


def cut_pileup(synth, sp, counts, rng):
    """A dense pileup cut to a sparse one in which barcode b keeps counts[b] of its pairs (the deepest first, the rest at random)."""
    B, S = sp.n_cells, sp.n_snps
    assert sp.pair_snp is None
    nrd = np.asarray(sp.pair_nrd).astype(np.int64)
    keep = np.zeros(B * S, dtype=bool)
    for b in range(B):
        n = nrd[b * S:(b + 1) * S]
        order = np.concatenate([np.flatnonzero(n > 255), rng.permutation(np.flatnonzero(n <= 255))])
        keep[b * S + order[:counts[b]]] = True
    return filter_pairs(synth, sp, keep)


def hand_pileup(synth, cells, S):
    """cells[b] = [(snp, read bytes), ...] in ascending SNP order -> a sparse SynthPileup."""
    po, ro, snps, nrds, rds = [0], [0], [], [], []
    for prs in cells:
        for s, rd in prs:
            snps.append(s); nrds.append(len(rd)); rds.append(np.asarray(rd, dtype=np.uint8))
        po.append(po[-1] + len(prs)); ro.append(ro[-1] + sum(len(rd) for _, rd in prs))
    nr = np.array(nrds, dtype=np.int64)
    t = np.diff(ro).astype(np.int32)
    return synth.SynthPileup(len(cells), S, np.array(po, dtype=np.int64), np.array(ro, dtype=np.int64), np.array(snps, dtype=np.int32),
                             nr.astype(np.uint8 if nr.max(initial=0) <= 255 else np.uint16),
                             np.concatenate(rds + [np.zeros(0, dtype=np.uint8)]).astype(np.uint8), t, t.copy(), t.copy(),
                             np.full((len(cells), 2), -1, dtype=np.int32))


def with_nrd(sp, dtype):
    import dataclasses
    return dataclasses.replace(sp, pair_nrd=np.asarray(sp.pair_nrd).astype(dtype))


def spike_rows(g, rng):
    """Rows that are all zero, that hold hard zeros, and one of float32 subnormals, at SNPs every barcode may cover."""
    g = g.copy()
    S, V, _ = g.shape
    sub = np.float32(1e-45)
    hard = [(1, 0, 0), (0, 0, 1), (0, 0.5, 0.5), (0.25, 0, 0.75)]
    for i, s in enumerate(rng.permutation(S)[:min(S, 10 + S // 8)]):
        v = i % V
        if i % 5 == 0:
            g[s, v] = 0
        elif i == 1:
            g[s, v] = (sub, 3 * sub, 0)
        else:
            g[s, v] = hard[i % 4]
    if S == 1:
        g[0, V - 1] = (sub, 3 * sub, 0)
    return g


ALT127, REF127 = (1 << 7) | 127, 127


def problems(engine, synth):
    """The shared inputs, by name (deterministic: every generator is seeded by the problem)."""
    out = {}

    def mixed(name, seed, quals, adversarial, deep, field, V=5, B=26, S=140, width=None, counts=None):
        rng = np.random.default_rng(seed)
        raw = synth.make_raw_genotypes(rng, S, V)
        g = spike_rows(QM.genotypes(engine, rng, raw.alleles, field), rng)
        sp = QM.mixed_depth_pileup(rng, raw.alleles, B, 1.0, quals=quals, dense=True, deep=deep, adversarial=adversarial)
        if counts is None:
            counts = np.concatenate([PAIR_COUNTS, PAIR_COUNTS, rng.integers(0, S + 1, size=B - 2 * len(PAIR_COUNTS))])
        sp = cut_pileup(synth, sp, np.asarray(counts), rng)
        if width is not None:
            sp = with_nrd(sp, width)
        out[name] = Problem(name, sp, g, deep=True)

    mixed("mix_full", 9101, "full", 0.15, 0, "GP")
    mixed("mix_edges", 9102, "edges", 0.3, 6, "GT")
    mixed("mix_max", 9103, "max", 0.5, 5, "PL", width=np.uint32)
    mixed("one_sample", 9104, "edges", 0.25, 0, "GT", V=1, B=9, counts=[0, 1, 63, 64, 65, 129, 17, 100, 140])
    assert out["mix_full"].sp.pair_nrd.dtype == np.uint8 and out["mix_edges"].sp.pair_nrd.dtype == np.uint16
    assert int(out["mix_edges"].sp.pair_nrd.max()) >= 256 and int(out["mix_max"].sp.pair_nrd.max()) >= 256

    for k, S in enumerate(PAIR_COUNTS[1:]):                     # dense layouts: every barcode has exactly S pairs
        rng = np.random.default_rng(9200 + S)
        V = 3
        raw = synth.make_raw_genotypes(rng, S, V)
        g = spike_rows(QM.genotypes(engine, rng, raw.alleles, ("GT", "GP", "PL")[k % 3]), rng)
        sp = QM.mixed_depth_pileup(rng, raw.alleles, 6, 1.0, quals=("full", "edges", "max")[k % 3], dense=True, deep=2 if S == 65 else 0,
                                   adversarial=0.3)
        if S == 129:
            sp = with_nrd(sp, np.uint32)
        out[f"dense_{S}"] = Problem(f"dense_{S}", sp, g, deep=S >= 63)
    assert out["dense_65"].sp.pair_nrd.dtype == np.uint16 and out["dense_64"].sp.pair_nrd.dtype == np.uint8

    # hand-built pairs: 7 / 8 / 9 reads (both sides of the rescale path's entry), 40 and 300 reads all ALT at quality 127 on a hom-REF row
    # (soft and hard), 16 and 24 reads whose products pass 2^-300 exactly at a check, a pair without stored reads, an unused barcode
    rng = np.random.default_rng(9300)
    S, V = 12, 3
    g = np.zeros((S, V, 3), dtype=np.float32)
    g[:, 0] = np.array([0.98, 0.015, 0.005], dtype=np.float32)             # hom-REF, soft
    g[:, 1] = (1, 0, 0)                                                      # hom-REF, hard zeros
    g[:, 2] = np.array([0.2, 0.5, 0.3], dtype=np.float32)
    g[9, :, :] = 0                                                           # a SNP whose every row is all zero
    g[10, 0] = (np.float32(1e-45), 0, 0)                                     # a float32 subnormal alone
    g[10, 1] = (0, np.float32(3e-45), np.float32(1e-45))
    rd = lambda n: ((rng.integers(0, 2, size=n) << 7) | rng.choice(synth.EDGE_QUALS, size=n)).astype(np.uint8)
    alt = lambda n: np.full(n, ALT127, dtype=np.uint8)
    cell = [(0, rd(7)), (1, rd(8)), (2, rd(9)), (3, alt(40)), (4, alt(300)), (5, alt(16)), (6, alt(24)), (7, np.zeros(0, dtype=np.uint8)),
            (8, alt(7)), (9, rd(5)), (10, alt(9)), (11, np.concatenate([alt(150), np.full(150, REF127, dtype=np.uint8)]))]
    out["edge"] = Problem("edge", hand_pileup(synth, [cell, cell, cell, [], cell[3:6]], S), g, deep=True)

    # tables under which a quality-0 read cannot be wrong: hard rows it contradicts have likelihood 0 (log arguments that are zero)
    mat, err = engine.phred_tables()
    mat, err = mat.copy(), err.copy()
    mat[0], err[0] = 1.0, 0.0
    g0 = np.zeros((8, 2, 3), dtype=np.float32)
    g0[:, :, 0] = 1.0
    alt0, ref30, alt30 = (1 << 7) | 0, 30, (1 << 7) | 30
    cells = [[(0, [alt0, ref30]), (1, [alt30]), (4, [ref30, alt0, ref30]), (6, [ref30] * 8 + [alt0])],
             [(2, [ref30, ref30]), (3, [ref30, ref30, alt0])], [(5, [alt0])], [(7, [ref30, alt30])]]
    out["zero"] = Problem("zero", hand_pileup(synth, cells, 8), g0, tables=(mat, err))

    # the refinement's shapes: samples of 0, 1, 63, 64, 65 and 130 assigned barcodes, S on both sides of the slab of 512
    for k, S in enumerate((511, 512, 513)):
        rng = np.random.default_rng(9400 + S)
        V, B = 6, 330
        raw = synth.make_raw_genotypes(rng, S, V)
        g = QM.genotypes(engine, rng, raw.alleles, "GT")
        sp = QM.mixed_depth_pileup(rng, raw.alleles, B, 0.04, quals=("edges", "full", "max")[k], deep=(3, 0, 4)[k], adversarial=0.15)
        snp = np.asarray(sp.pair_snp)
        keep = snp != 5                                           # SNP 5: no slot; SNP 6: a single slot; so for the last SNP
        for one in (6, S - 1):
            keep &= (snp != one) | (np.arange(len(snp)) == np.flatnonzero(snp == one)[0])
        sp = filter_pairs(synth, sp, keep)
        if k == 2:
            sp = with_nrd(sp, np.uint32)
        out[f"slab_{S}"] = Problem(f"slab_{S}", sp, g)
    return out


def amb_freq(p, seed=1):
    """a[S] in [0, 1] with exact zeros and ones."""
    S = p.g.shape[0]
    a = np.random.default_rng(9500 + seed + S).uniform(0.0, 1.0, size=S)
    a[::7] = 0.0
    a[3::11] = 1.0
    return a


def assignment(p, seed=2):
    """assign[B]: the barcode's own sample (barcode b is sample b mod V in these pileups), a fifth unused."""
    B = p.sp.n_cells
    rng = np.random.default_rng(9600 + seed + B)
    a = (np.arange(B) % p.V).astype(np.int32)
    a[rng.random(B) < 0.2] = -1
    if p.name == "edge":
        a[:] = [0, 1, 2, -1, 1]
    if p.name == "zero":
        a[:] = [0, 0, 1, 1]
    return a


GRIDS = {1: np.array([0.13]), 2: np.array([0.0, 1.0]), 3: np.array([0.0, 0.2, 1.0]), 64: np.linspace(0.0, 0.5, 64), 65: np.linspace(0.0, 1.0, 65)}
AMBIENT_CASES = [("mix_full", 65), ("mix_edges", 64), ("mix_max", 1), ("one_sample", 3), ("dense_1", 2), ("dense_63", 3), ("dense_64", 1),
                 ("dense_65", 65), ("dense_129", 2), ("edge", 65), ("zero", 2)]


def candidates(p, Cn, seed=3):
    """cand[B][Cn][2]: random pairs of different samples, one slot in six unused (v1 = -1)."""
    B, V = p.sp.n_cells, p.V
    rng = np.random.default_rng(9700 + seed + 31 * Cn + B)
    v1 = rng.integers(0, V, size=(B, Cn))
    v2 = (v1 + 1 + rng.integers(0, V - 1, size=(B, Cn))) % V
    v1 = np.where(rng.random((B, Cn)) < 1 / 6, -1, v1)
    cand = np.stack([v1, v2], axis=2).astype(np.int32)
    if p.name == "edge":                                      # every ordered pair of the three rows on the hand-built barcodes
        prs = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1), (-1, 0), (0, 1)]
        cand[:] = np.array(prs[:Cn], dtype=np.int32)[None]
    return cand


ALPHAS = {1: np.array([0.37]), 3: np.array([0.0, 0.37, 0.5])}
# (problem, candidate slots, alphas, grid points): every slot count 1..8 (k_ambient_dbl<1, 64>, <2, 64>, <4, 32> for 3 and 4, <8, 32> above)
AMBIENT_DBL_CASES = [("mix_edges", 1, 3, 3), ("mix_edges", 2, 1, 65), ("mix_full", 3, 1, 2), ("mix_max", 4, 3, 1), ("mix_full", 5, 1, 3),
                     ("dense_65", 6, 1, 2), ("dense_129", 7, 1, 1), ("mix_edges", 8, 1, 64), ("dense_1", 2, 3, 2), ("dense_63", 3, 1, 3),
                     ("dense_64", 8, 3, 2), ("edge", 8, 3, 65), ("edge", 4, 1, 3), ("zero", 1, 1, 2)]


def hypotheses(p, seed=4):
    """(hyp[B][2], alpha[B], rho[B]): singlets and (for V > 1) doublets of the barcode's sample, one in six unused."""
    B, V = p.sp.n_cells, p.V
    rng = np.random.default_rng(9800 + seed + B)
    v1 = np.arange(B) % V
    v2 = np.where((rng.random(B) < 0.5) & (V > 1), (v1 + 1 + rng.integers(0, max(V - 1, 1), size=B)) % V, -1)
    v1 = np.where(rng.random(B) < 1 / 6, -1, v1)
    hyp = np.stack([v1, v2], axis=1).astype(np.int32)
    n = len(PAIR_COUNTS)
    if V > 1 and B >= 2 * n:                                    # the barcodes of the exact pair counts: once as singlets, once as doublets
        hyp[:n] = [(b % V, -1) for b in range(n)]
        hyp[n:2 * n] = [(b % V, (b + 1) % V) for b in range(n)]
    alpha = rng.choice([0.0, 0.5, 0.37], size=B)
    rho = rng.choice([0.0, 0.05, 0.3, 1.0], size=B)
    if p.name == "edge":
        hyp[:] = [(0, -1), (1, 2), (2, 0), (0, 1), (1, -1)]
        alpha[:] = [0.0, 0.37, 0.5, 0.37, 0.0]
    if p.name == "zero":
        hyp[:] = [(0, -1), (0, 1), (1, -1), (1, 0)]
        alpha[:] = [0.0, 0.5, 0.0, 0.37]
        rho[:] = 0.0
    return hyp, alpha, rho


# (problem, M, rho given): every M for singlets and doublets (both kinds of barcode are in every call), rho = None against given
FIT_CASES = [("mix_edges", 1, True), ("mix_edges", 2, True), ("mix_edges", 3, True), ("mix_edges", 4, True), ("mix_edges", 5, True),
             ("mix_edges", 8, True), ("mix_full", 1, False), ("mix_full", 4, False), ("mix_full", 8, False), ("mix_max", 2, True),
             ("mix_max", 8, False), ("one_sample", 3, True), ("one_sample", 8, False), ("dense_1", 4, True), ("dense_63", 5, False),
             ("dense_64", 8, True), ("dense_65", 2, True), ("dense_129", 8, True), ("dense_129", 3, False), ("edge", 8, True), ("edge", 4, False),
             ("zero", 2, False), ("zero", 8, False)]


def refine_assignment(p, seed=5):
    """assign[B] with samples of 0, 1, 63, 64, 65 and 130 barcodes (slab problems); the barcode's own sample elsewhere."""
    B, V = p.sp.n_cells, p.V
    if not p.name.startswith("slab_"):
        return assignment(p, seed)
    rng = np.random.default_rng(9900 + seed + B)
    sizes = (0, 1, 63, 64, 65, 130)
    a = np.concatenate([np.full(n, v) for v, n in enumerate(sizes)] + [np.full(B - sum(sizes), -1)]).astype(np.int32)
    return rng.permutation(a)


REFINE_CASES = ["slab_511", "slab_512", "slab_513", "mix_full", "mix_edges", "mix_max", "one_sample", "dense_1", "dense_63", "dense_64",
                "dense_65", "dense_129", "edge"]


def mstep_weights(p, Cn, seed=6):
    """w[B][Cn] float64: ordinary values, exact 0 and 1, 1e-300; a column without weight when there are three or more."""
    B = p.sp.n_cells
    rng = np.random.default_rng(9950 + seed + Cn + B)
    w = rng.dirichlet(np.ones(max(Cn, 2)), size=B)[:, :Cn] * rng.random((B, 1))
    k = rng.random((B, Cn))
    w[k < 0.1] = 0.0
    w[(k >= 0.1) & (k < 0.2)] = 1.0
    w[(k >= 0.2) & (k < 0.3)] = 1e-300
    if Cn >= 3:
        w[:, 1] = 0.0
    w[rng.random(B) < 0.1] = 0.0
    return np.ascontiguousarray(w)


MSTEP_CASES = [("slab_511", 1), ("slab_512", 3), ("slab_513", 70), ("mix_edges", 3), ("dense_65", 70), ("edge", 1)]
