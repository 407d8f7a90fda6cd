"""Per-barcode ambient RNA contamination ("soup") from the allele data the engine already holds.

Soup is the average of many lysed cells, so at SNP i its reads show ALT with a fixed frequency a_i.  A droplet called as sample v with
a fraction rho of soup reads has, at SNP i, ALT probability p_g(rho) = (1 - rho) g / 2 + rho a_i under each genotype g of v.  The engine
computes the log-likelihood of every assigned barcode's reads over a grid of rho (Engine.ambient_profile, dmx_engine_ambient; DESIGN.md
section 14); this module builds a, reads the profile into per-barcode estimates and a pool estimate, and writes them:

  <prefix>.ambient.tsv       BARCODE SM_ID N.SNP N.READ RHO RHO.LO RHO.HI LLK.RHO LLK.0 LLR — one row per assigned barcode
  <prefix>.ambient_pool.tsv  RHO LLK per grid point: the sum of the assigned barcodes' profiles, then the pool estimate

RHO is the grid point of the highest LL (the lowest one on ties), RHO.LO / RHO.HI the smallest and largest grid points whose LL is within
1.92 (half the 95 % chi-square quantile of one degree of freedom) of that maximum, LLK.0 the LL at rho = 0 and LLR = LLK.RHO - LLK.0.
A doublet called as a singlet also looks like a high-rho singlet: a high RHO is a QC signal, not a proof of soup.

    python -m demuxlet_amd.ambient --pileup <x>.pileup.txt --out <prefix> [--best <x>.best] [--min-prb P] [--ambient reads|genotypes|census]
        [--grid-max 0.5] [--grid-step 0.01 | --grid R ...] [--alpha A ...] [--doublets [--dbl-alpha A ...]] [--fast] [--gpu G]

reads the dump that `demuxlet --pileup-only` writes.  Without --best, the unchanged demultiplexing pass runs first and writes
<prefix>.best/.single/.sing2; its singlets are the barcodes profiled.

The plain pass has no soup term in its doublet grid: a soupy singlet's foreign alleles can only be explained by a second donor, and it
is called DBL-.  With --doublets [--dbl-alpha A ...] every barcode of the `.best` is called again with soup in BOTH hypotheses
(ambient_calls_run): the singlet profiles of SNG.1ST and SNG.2ND, and the ambient-aware doublet profile
(Engine.ambient_doublet_profile) of the pairs (DBL.1ST, DBL.2ND) and (SNG.1ST, SNG.2ND) over the mixing shares alpha.  LLK.SNG1 / LLK.SNG2
are the maxima over rho, LLK.DBL the maximum over candidates, alpha and rho (lowest index on ties), and the reference's rule
(cmd_cram_demuxlet.cpp:835-858, margin 2) decides: DBL if LLK.DBL > LLK.SNG1 + 2, else SNG if LLK.SNG1 > LLK.SNG2 + 2, else AMB.  The
shares are the run's --alpha values above 0 unless --dbl-alpha is given: at alpha = 0 the doublet model IS the singlet one, so it is
left out (as the reference leaves n = 0 out of its doublet search).

  <prefix>.ambient_calls.tsv BARCODE BEST CALL SNG.1ST RHO.SNG1 LLK.SNG1 SNG.2ND RHO.SNG2 LLK.SNG2 DBL.1ST DBL.2ND ALPHA RHO.DBL LLK.DBL
                             LLR N.SNP N.READ — one row per barcode of the `.best`, in byte-wise barcode order; BEST is the plain
                             call, CALL the new one (SNG-x, DBL-x-y-alpha, AMB-x-y-j/k), LLR = LLK.DBL - LLK.SNG1

Without --doublets nothing of this is computed or written."""
from __future__ import annotations

import argparse
import sys
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import capi, engine, refine

MAX_GRID = 256              # dmx_engine_ambient's longest grid
CI_DROP = 1.92              # RHO.LO / RHO.HI: grid points with LL >= max - CI_DROP
AMBIENT_HEADER = "BARCODE\tSM_ID\tN.SNP\tN.READ\tRHO\tRHO.LO\tRHO.HI\tLLK.RHO\tLLK.0\tLLR\n"
POOL_HEADER = "RHO\tLLK\n"
CALLS_HEADER = ("BARCODE\tBEST\tCALL\tSNG.1ST\tRHO.SNG1\tLLK.SNG1\tSNG.2ND\tRHO.SNG2\tLLK.SNG2\tDBL.1ST\tDBL.2ND\tALPHA\tRHO.DBL\tLLK.DBL\t"
                "LLR\tN.SNP\tN.READ\n")
CALL_MARGIN = 2.0           # the reference's margin (cmd_cram_demuxlet.cpp:840, :847)
MAX_DBL_ALPHA = 8           # dmx_engine_ambient_doublet's longest alpha grid
CALL_SNG, CALL_DBL, CALL_AMB = 0, 1, 2


def default_grid(grid_max: float = 0.5, grid_step: float = 0.01) -> np.ndarray:
    """0, step, 2 step, ... up to grid_max (51 points by default)."""
    if not (grid_step > 0.0) or not (0.0 <= grid_max <= 1.0):
        raise ValueError(f"grid: step {grid_step} must be > 0 and max {grid_max} in [0, 1]")
    n = int(np.floor(grid_max / grid_step + 1e-9)) + 1
    return check_grid(np.round(np.arange(n) * grid_step, 12))


def check_grid(grid) -> np.ndarray:
    g = np.ascontiguousarray(grid, dtype=np.float64)
    if g.ndim != 1 or not 1 <= len(g) <= MAX_GRID:
        raise ValueError(f"grid: 1 to {MAX_GRID} points, got {g.size}")
    if not np.all((g >= 0.0) & (g <= 1.0)):
        raise ValueError("grid: every point must be in [0, 1]")
    if len(g) > 1 and not np.all(np.diff(g) > 0.0):
        raise ValueError("grid: points must be strictly ascending")
    return g


def check_ambient(a, n_snps: int) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (n_snps,):
        raise ValueError(f"ambient: {a.shape} for {n_snps} SNPs")
    if not np.all((a >= 0.0) & (a <= 1.0)):
        raise ValueError("ambient: every frequency must be in [0, 1]")
    return a


def check_assign(assign, n_cells: int, n_samples: int) -> np.ndarray:
    a = np.ascontiguousarray(assign, dtype=np.int32)
    if a.shape != (n_cells,):
        raise ValueError(f"assign: {a.shape} for {n_cells} barcodes")
    if a.size and (a.min() < -1 or a.max() >= n_samples):
        raise ValueError(f"assign: sample indices must be in [-1, {n_samples})")
    return a


def ambient_from_counts(n_ref, n_alt) -> np.ndarray:
    """a_i = (n_alt + 1) / (n_ref + n_alt + 2): the pooled ALT fraction of every barcode's stored reads."""
    r = np.asarray(n_ref, dtype=np.float64)
    x = np.asarray(n_alt, dtype=np.float64)
    return (x + 1.0) / (r + x + 2.0)


def ambient_from_genotypes(g, assign) -> np.ndarray:
    """a_i = sum over v of pi_v (gp[i][v][1] / 2 + gp[i][v][2]), pi_v the fraction of the assigned barcodes called v."""
    g = np.asarray(g, dtype=np.float64)
    a = np.asarray(assign)
    n = np.bincount(a[a >= 0], minlength=g.shape[1]).astype(np.float64)
    if n.sum() == 0:
        raise ValueError("ambient from genotypes: no assigned barcode")
    pi = n / n.sum()
    return np.clip((g[:, :, 1] * 0.5 + g[:, :, 2]) @ pi, 0.0, 1.0)


def ambient_from_reads(eng: engine.Engine, g: np.ndarray) -> np.ndarray:
    """ambient_from_counts over the engine's staged pileup: one refinement with every barcode in column 0 (as cluster.py's prior)."""
    _, _, n_ref, n_alt, _ = eng.refine_genotypes(np.zeros(eng.B, dtype=np.int32), g)
    return ambient_from_counts(n_ref[:, 0], n_alt[:, 0])


def ambient_from_census(eng: engine.Engine, g: np.ndarray) -> np.ndarray:
    """a_i = sum over v of w_v d_iv with w the maximum-likelihood donor shares of ALL barcodes' reads (Engine.census with one group;
    census.py): the shares follow the reads, so RNA content and which donor's cells lysed are in them, and the
    profile has the variance of V estimated shares at every SNP, however few reads it has.  0.5 at a SNP where a donor's genotype
    row is all zero (the census leaves such SNPs out)."""
    from . import census
    w = eng.census(np.zeros(eng.B, dtype=np.int32), n_groups=1)["w"][0]
    return np.clip(np.nan_to_num(census.ambient_profile(w, g), nan=0.5), 0.0, 1.0)


def _ambient_builder(ambient: str, eng: engine.Engine, g: np.ndarray, assign_fn) -> np.ndarray:
    if ambient == "reads":
        return ambient_from_reads(eng, g)
    if ambient == "census":
        return ambient_from_census(eng, g)
    return ambient_from_genotypes(g, assign_fn())


@dataclass
class Summary:
    """Per-barcode estimates from a profile ll[B][Q] (rows of unassigned barcodes are meaningless)."""
    rho: np.ndarray          # grid point of the highest LL, lowest on ties
    rho_lo: np.ndarray       # smallest grid point with LL >= max - CI_DROP
    rho_hi: np.ndarray       # largest one
    llk_rho: np.ndarray
    llk_0: np.ndarray        # LL at rho = 0 (NaN when the grid has no 0)
    llr: np.ndarray


def summarize(ll: np.ndarray, grid) -> Summary:
    ll = np.asarray(ll, dtype=np.float64)
    g = check_grid(grid)
    if ll.ndim != 2 or ll.shape[1] != len(g):
        raise ValueError(f"profile {ll.shape} for a grid of {len(g)}")
    B = ll.shape[0]
    top = np.argmax(ll, axis=1) if B else np.zeros(0, dtype=np.int64)
    mx = ll[np.arange(B), top]
    inside = ll >= (mx - CI_DROP)[:, None]
    lo = np.argmax(inside, axis=1) if B else top
    hi = len(g) - 1 - np.argmax(inside[:, ::-1], axis=1) if B else top
    l0 = ll[:, 0] if g[0] == 0.0 else np.full(B, np.nan)
    return Summary(g[top], g[lo], g[hi], mx, l0, mx - l0)


def pool_profile(ll: np.ndarray, assign) -> np.ndarray:
    """sum over the assigned barcodes of ll[b], added serially in ascending cell id."""
    ll = np.asarray(ll, dtype=np.float64)
    sel = ll[np.asarray(assign) >= 0]
    if len(sel) == 0:
        return np.zeros(ll.shape[1])
    return np.cumsum(sel, axis=0)[-1]


def write_ambient_tsv(path: str, barcodes: Sequence[str], sample_ids: Sequence[str], assign, n_snp, n_read, s: Summary) -> None:
    """One row per assigned barcode, in cell id order."""
    with open(path, "w") as f:
        f.write(AMBIENT_HEADER)
        for b in np.flatnonzero(np.asarray(assign) >= 0):
            f.write(f"{barcodes[b]}\t{sample_ids[int(assign[b])]}\t{int(n_snp[b])}\t{int(n_read[b])}\t{s.rho[b]:.4f}\t{s.rho_lo[b]:.4f}\t"
                    f"{s.rho_hi[b]:.4f}\t{s.llk_rho[b]:.5f}\t{s.llk_0[b]:.5f}\t{s.llr[b]:.5f}\n")


def write_pool_tsv(path: str, grid, pool: np.ndarray) -> float:
    """RHO LLK per grid point, then a `#RHO.POOL` line with the argmax (lowest on ties); returns it."""
    g = check_grid(grid)
    est = float(g[int(np.argmax(pool))])
    with open(path, "w") as f:
        f.write(POOL_HEADER)
        for r, x in zip(g, pool):
            f.write(f"{r:.4f}\t{x:.5f}\n")
        f.write(f"#RHO.POOL\t{est:.4f}\n")
    return est


def ambient_run(store_or_pileup, g: np.ndarray, sample_ids: Sequence[str], out_prefix: str, best: Optional[str] = None, ambient="reads",
                grid=None, min_prb: float = 0.0, alphas: Sequence[float] = (0.0, 0.5), barcodes: Optional[Sequence[str]] = None,
                device: int = 0, mode: int = capi.DMX_MODE_STRICT, **demuxlet_run_kwargs):
    """Profile the singlets of `best` (a `.best` path) against genotype matrix g.  Without `best`, the unchanged demuxlet_run writes
    <out_prefix>.best/.single/.sing2 first and its `.best` is used.  `ambient` is "reads", "genotypes", "census" or an array of n_snps frequencies.
    `store_or_pileup` is a Store, or a HostPileup with barcodes=... as for demuxlet_run.  Writes <out_prefix>.ambient.tsv and
    .ambient_pool.tsv; returns a dict with the profile, counts, summary, pool profile and pool estimate."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    grid = default_grid() if grid is None else check_grid(grid)
    if isinstance(ambient, str) and ambient not in ("reads", "genotypes", "census"):
        raise ValueError(f"ambient: 'reads', 'genotypes', 'census' or an array, not {ambient!r}")
    if isinstance(store_or_pileup, engine.HostPileup):
        pl = store_or_pileup
        if barcodes is None:
            raise ValueError("ambient_run: a HostPileup needs barcodes=")
    else:
        pl, barcodes = store_or_pileup.freeze(), store_or_pileup.barcodes()
    if g.ndim != 3 or g.shape[0] != pl.n_snps or g.shape[1] != len(sample_ids) or g.shape[2] != 3:
        raise ValueError(f"genotype matrix {g.shape} for {pl.n_snps} SNPs and {len(sample_ids)} samples")
    if not isinstance(ambient, str):
        ambient = check_ambient(ambient, pl.n_snps)
    if best is None:
        engine.demuxlet_run(pl, g, sample_ids, alphas, out_prefix, barcodes=barcodes, device=device, mode=mode, **demuxlet_run_kwargs)
        best = out_prefix + ".best"
    assign = refine.assignments_from_best(best, sample_ids, barcodes, min_prb)
    eng = engine.Engine(len(sample_ids), alphas, device=device, mode=mode)
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        if isinstance(ambient, str):
            a = _ambient_builder(ambient, eng, g, lambda: assign)
        else:
            a = ambient
        ll, n_snp, n_read = eng.ambient_profile(assign, a, grid)
    finally:
        eng.close()
    s = summarize(ll, grid)
    pool = pool_profile(ll, assign)
    write_ambient_tsv(out_prefix + ".ambient.tsv", barcodes, sample_ids, assign, n_snp, n_read, s)
    est = write_pool_tsv(out_prefix + ".ambient_pool.tsv", grid, pool)
    return dict(assign=assign, ambient=a, grid=grid, ll=ll, n_snp=n_snp, n_read=n_read, summary=s, pool=pool, pool_rho=est)


def check_dbl_alphas(alphas) -> np.ndarray:
    """The mixing shares of the ambient-aware doublet profile: 1 to 8, strictly ascending, in (0, 1]."""
    al = np.ascontiguousarray(alphas, dtype=np.float64)
    if al.ndim != 1 or not 1 <= len(al) <= MAX_DBL_ALPHA:
        raise ValueError(f"doublet alphas: 1 to {MAX_DBL_ALPHA} values, got {al.size}")
    if not np.all((al > 0.0) & (al <= 1.0)):
        raise ValueError("doublet alphas: every value must be in (0, 1] (at 0 the doublet model is the singlet one)")
    if len(al) > 1 and not np.all(np.diff(al) > 0.0):
        raise ValueError("doublet alphas: values must be strictly ascending")
    return al


def dbl_alphas_from_run(alphas) -> np.ndarray:
    """The run's --alpha values above 0, sorted."""
    al = np.unique(np.asarray(alphas, dtype=np.float64))
    return check_dbl_alphas(al[al > 0.0])


@dataclass
class BestRows:
    """Every row of a `.best` by cell id: the plain call and the four sample indices (-1: no row for this barcode)."""
    best: list               # BEST strings, "" without a row
    sng1: np.ndarray
    sng2: np.ndarray
    dbl1: np.ndarray
    dbl2: np.ndarray

    @property
    def has_row(self) -> np.ndarray:
        return self.sng1 >= 0


def read_best_rows(path: str, sample_ids: Sequence[str], barcodes: Sequence[str]) -> BestRows:
    """All rows of a `.best` (refine.assignments_from_best keeps the SNG- ones only)."""
    smap = {s: j for j, s in enumerate(sample_ids)}
    cmap = {b: c for c, b in enumerate(barcodes)}
    B = len(barcodes)
    best = [""] * B
    idx = {n: np.full(B, -1, dtype=np.int32) for n in ("SNG.1ST", "SNG.2ND", "DBL.1ST", "DBL.2ND")}
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        col = {n: i for i, n in enumerate(head)}
        for n in ("BARCODE", "BEST", *idx):
            if n not in col:
                raise ValueError(f"{path}: no {n} column")
        for line in f:
            t = line.rstrip("\n").split("\t")
            if len(t) < len(head):
                continue
            c = cmap.get(t[col["BARCODE"]])
            if c is None:
                raise ValueError(f"{path}: barcode {t[col['BARCODE']]!r} not in this job")
            best[c] = t[col["BEST"]]
            for n, arr in idx.items():
                j = smap.get(t[col[n]])
                if j is None:
                    raise ValueError(f"{path}: sample {t[col[n]]!r} not in this job")
                arr[c] = j
    return BestRows(best, idx["SNG.1ST"], idx["SNG.2ND"], idx["DBL.1ST"], idx["DBL.2ND"])


def candidates_from_best(rows: BestRows) -> np.ndarray:
    """cand[B][2][2] for Engine.ambient_doublet_profile: slot 0 = (DBL.1ST, DBL.2ND), slot 1 = (SNG.1ST, SNG.2ND) when that is a
    different unordered pair; a slot whose two samples coincide, or of a barcode without a row, is unused (-1, -1)."""
    B = len(rows.sng1)
    cand = np.full((B, 2, 2), -1, dtype=np.int32)
    ok0 = rows.has_row & (rows.dbl1 >= 0) & (rows.dbl2 >= 0) & (rows.dbl1 != rows.dbl2)
    cand[ok0, 0, 0] = rows.dbl1[ok0]
    cand[ok0, 0, 1] = rows.dbl2[ok0]
    same = ((rows.sng1 == rows.dbl1) & (rows.sng2 == rows.dbl2)) | ((rows.sng1 == rows.dbl2) & (rows.sng2 == rows.dbl1))
    ok1 = rows.has_row & (rows.sng2 >= 0) & (rows.sng1 != rows.sng2) & ~(ok0 & same)
    cand[ok1, 1, 0] = rows.sng1[ok1]
    cand[ok1, 1, 1] = rows.sng2[ok1]
    return cand


def decide(llk_sng1, llk_sng2, llk_dbl) -> np.ndarray:
    """The reference's rule on the three maxima: CALL_DBL if LLK.DBL > LLK.SNG1 + 2, else CALL_SNG if LLK.SNG1 > LLK.SNG2 + 2, else
    CALL_AMB.  A comparison that ties at the margin is not won."""
    s1, s2, d = (np.asarray(x, dtype=np.float64) for x in (llk_sng1, llk_sng2, llk_dbl))
    return np.where(d > s1 + CALL_MARGIN, CALL_DBL, np.where(s1 > s2 + CALL_MARGIN, CALL_SNG, CALL_AMB)).astype(np.int32)


@dataclass
class Calls:
    """ambient-aware calls per cell id (meaningless where the `.best` has no row)."""
    call: np.ndarray         # CALL_SNG / CALL_DBL / CALL_AMB
    rho_sng1: np.ndarray
    llk_sng1: np.ndarray
    rho_sng2: np.ndarray
    llk_sng2: np.ndarray
    dbl1: np.ndarray         # the doublet candidate of the highest LL (-1: the barcode had no candidate pair)
    dbl2: np.ndarray
    alpha: np.ndarray
    rho_dbl: np.ndarray
    llk_dbl: np.ndarray
    llr: np.ndarray


def make_calls(rows: BestRows, cand: np.ndarray, ll_sng1: np.ndarray, ll_sng2: np.ndarray, ll_dbl: np.ndarray, dbl_alphas, grid) -> Calls:
    """Maxima of the two singlet profiles [B][Q] and of the doublet profile [B][C][A][Q] (lowest index on ties, in candidate, alpha, rho
    order; unused slots and an absent SNG.2ND count as -inf), then decide()."""
    g = check_grid(grid)
    al = np.asarray(dbl_alphas, dtype=np.float64)
    B = len(rows.sng1)
    rb = np.arange(B)
    t1 = np.argmax(ll_sng1, axis=1) if B else np.zeros(0, dtype=np.int64)
    t2 = np.argmax(ll_sng2, axis=1) if B else np.zeros(0, dtype=np.int64)
    l1 = ll_sng1[rb, t1]
    l2 = np.where(rows.sng2 >= 0, ll_sng2[rb, t2], -np.inf)
    Cn, A, Q = ll_dbl.shape[1:]
    x = np.where((cand[:, :, 0] >= 0)[:, :, None, None], ll_dbl, -np.inf).reshape(B, Cn * A * Q)
    td = np.argmax(x, axis=1) if B else np.zeros(0, dtype=np.int64)
    ld = x[rb, td]
    c, n, q = td // (A * Q), (td // Q) % A, td % Q
    none = ~np.isfinite(ld) & ~(cand[:, :, 0] >= 0).any(axis=1)
    return Calls(decide(l1, l2, ld), g[t1], l1, g[t2], l2, np.where(none, -1, cand[rb, c, 0]), np.where(none, -1, cand[rb, c, 1]),
                 al[n], g[q], ld, ld - l1)


def call_string(k: int, rows: BestRows, calls: Calls, sample_ids: Sequence[str]) -> str:
    """SNG-x / DBL-x-y-alpha / AMB-x-y-j/k in the reference's spelling (cmd_cram_demuxlet.cpp:840-858)."""
    name = lambda j: sample_ids[int(j)] if j >= 0 else "."
    if calls.call[k] == CALL_DBL:
        return f"DBL-{name(calls.dbl1[k])}-{name(calls.dbl2[k])}-{calls.alpha[k]:.3f}"
    if calls.call[k] == CALL_SNG:
        return f"SNG-{name(rows.sng1[k])}"
    return f"AMB-{name(rows.sng1[k])}-{name(rows.sng2[k])}-{name(calls.dbl1[k])}/{name(calls.dbl2[k])}"


def write_calls_tsv(path: str, barcodes: Sequence[str], sample_ids: Sequence[str], rows: BestRows, calls: Calls, n_snp, n_read) -> None:
    """One row per barcode of the `.best`, in ascending byte-wise barcode order (the writers' order)."""
    name = lambda j: sample_ids[int(j)] if j >= 0 else "."
    order = sorted(np.flatnonzero(rows.has_row), key=lambda k: barcodes[k].encode())
    with open(path, "w") as f:
        f.write(CALLS_HEADER)
        for k in order:
            c = calls
            f.write(f"{barcodes[k]}\t{rows.best[k]}\t{call_string(k, rows, c, sample_ids)}\t{name(rows.sng1[k])}\t{c.rho_sng1[k]:.4f}\t"
                    f"{c.llk_sng1[k]:.5f}\t{name(rows.sng2[k])}\t{c.rho_sng2[k]:.4f}\t{c.llk_sng2[k]:.5f}\t{name(c.dbl1[k])}\t{name(c.dbl2[k])}\t"
                    f"{c.alpha[k]:.3f}\t{c.rho_dbl[k]:.4f}\t{c.llk_dbl[k]:.5f}\t{c.llr[k]:.5f}\t{int(n_snp[k])}\t{int(n_read[k])}\n")


def ambient_calls_run(store_or_pileup, g: np.ndarray, sample_ids: Sequence[str], out_prefix: str, best: Optional[str] = None, ambient="reads",
                      grid=None, alphas: Sequence[float] = (0.0, 0.5), dbl_alphas=None, barcodes: Optional[Sequence[str]] = None,
                      device: int = 0, mode: int = capi.DMX_MODE_STRICT, **demuxlet_run_kwargs):
    """Call every barcode of `best` (a `.best` path) again with soup in the singlet and in the doublet hypothesis.  Without `best`, the
    unchanged demuxlet_run writes <out_prefix>.best/.single/.sing2 first.  `dbl_alphas` defaults to the values of `alphas` above 0;
    the other arguments are ambient_run's.  Writes <out_prefix>.ambient_calls.tsv; returns a dict with the rows, candidates, the three
    profiles and the calls."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    grid = default_grid() if grid is None else check_grid(grid)
    dal = dbl_alphas_from_run(alphas) if dbl_alphas is None else check_dbl_alphas(dbl_alphas)
    if isinstance(ambient, str) and ambient not in ("reads", "genotypes", "census"):
        raise ValueError(f"ambient: 'reads', 'genotypes', 'census' or an array, not {ambient!r}")
    if isinstance(store_or_pileup, engine.HostPileup):
        pl = store_or_pileup
        if barcodes is None:
            raise ValueError("ambient_calls_run: a HostPileup needs barcodes=")
    else:
        pl, barcodes = store_or_pileup.freeze(), store_or_pileup.barcodes()
    if g.ndim != 3 or g.shape[0] != pl.n_snps or g.shape[1] != len(sample_ids) or g.shape[2] != 3:
        raise ValueError(f"genotype matrix {g.shape} for {pl.n_snps} SNPs and {len(sample_ids)} samples")
    if not isinstance(ambient, str):
        ambient = check_ambient(ambient, pl.n_snps)
    if best is None:
        engine.demuxlet_run(pl, g, sample_ids, alphas, out_prefix, barcodes=barcodes, device=device, mode=mode, **demuxlet_run_kwargs)
        best = out_prefix + ".best"
    rows = read_best_rows(best, sample_ids, barcodes)
    cand = candidates_from_best(rows)
    eng = engine.Engine(len(sample_ids), alphas, device=device, mode=mode)
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        if isinstance(ambient, str):
            a = _ambient_builder(ambient, eng, g, lambda: refine.assignments_from_best(best, sample_ids, barcodes))
        else:
            a = ambient
        ll1, n_snp, n_read = eng.ambient_profile(rows.sng1, a, grid)
        ll2, _, _ = eng.ambient_profile(rows.sng2, a, grid)
        lld, _, _ = eng.ambient_doublet_profile(cand, dal, a, grid)
    finally:
        eng.close()
    calls = make_calls(rows, cand, ll1, ll2, lld, dal, grid)
    write_calls_tsv(out_prefix + ".ambient_calls.tsv", barcodes, sample_ids, rows, calls, n_snp, n_read)
    return dict(rows=rows, cand=cand, ambient=a, grid=grid, dbl_alphas=dal, ll_sng1=ll1, ll_sng2=ll2, ll_dbl=lld, n_snp=n_snp, n_read=n_read,
                calls=calls)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.ambient", description="per-barcode ambient RNA contamination from allele data")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.ambient.tsv, <out>.ambient_pool.tsv (and <out>.best/... without --best)")
    ap.add_argument("--best", help="a .best of this pileup: its singlets are profiled (default: run the demultiplexing pass first)")
    ap.add_argument("--min-prb", type=float, default=0.0, help="use only singlets with PRB.SNG1 >= this (default: all SNG- calls)")
    ap.add_argument("--ambient", choices=("reads", "genotypes", "census"), default="reads",
                    help="soup ALT frequency: pooled reads of every barcode (default), the singlet-weighted genotype mean, or the genotype "
                         "mean weighted by the donor shares of all barcodes' reads (census.py)")
    ap.add_argument("--grid-max", type=float, default=0.5, help="largest contamination fraction of the default grid (default 0.5)")
    ap.add_argument("--grid-step", type=float, default=0.01, help="step of the default grid (default 0.01)")
    ap.add_argument("--grid", type=float, nargs="+", help="explicit grid of contamination fractions (replaces --grid-max / --grid-step)")
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.0, 0.5], help="doublet grid of the demultiplexing pass (default 0 0.5)")
    ap.add_argument("--doublets", action="store_true",
                    help="also call every barcode of the .best again with soup in the singlet and the doublet model: <out>.ambient_calls.tsv")
    ap.add_argument("--dbl-alpha", type=float, nargs="+",
                    help="mixing shares of the ambient-aware doublet model, in (0, 1] (default: the --alpha values above 0); needs --doublets")
    ap.add_argument("--fast", action="store_true", help="DMX_MODE_FAST for the demultiplexing pass")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    if not 0.0 <= a.min_prb <= 1.0:
        ap.error("--min-prb must be in [0, 1]")
    try:
        a.grid = check_grid(a.grid) if a.grid is not None else default_grid(a.grid_max, a.grid_step)
    except ValueError as ex:
        ap.error(str(ex))
    if a.dbl_alpha is not None and not a.doublets:
        ap.error("--dbl-alpha needs --doublets")
    if a.doublets:
        try:
            a.dbl_alpha = check_dbl_alphas(a.dbl_alpha) if a.dbl_alpha is not None else dbl_alphas_from_run(a.alpha)
        except ValueError as ex:
            ap.error(str(ex))
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    d = refine.read_pileup_txt(a.pileup)
    r = ambient_run(d.pileup, d.g, d.sample_ids, a.out, best=a.best, ambient=a.ambient, grid=a.grid, min_prb=a.min_prb, alphas=a.alpha,
                    barcodes=d.barcodes, device=a.gpu, mode=capi.DMX_MODE_FAST if a.fast else capi.DMX_MODE_STRICT)
    print(f"{int((r['assign'] >= 0).sum())} barcodes profiled; pool rho = {r['pool_rho']:.4f}", file=sys.stderr)
    if a.doublets:
        c = ambient_calls_run(d.pileup, d.g, d.sample_ids, a.out, best=a.best if a.best else a.out + ".best", ambient=r["ambient"], grid=a.grid,
                              alphas=a.alpha, dbl_alphas=a.dbl_alpha, barcodes=d.barcodes, device=a.gpu,
                              mode=capi.DMX_MODE_FAST if a.fast else capi.DMX_MODE_STRICT)
        n = np.bincount(c["calls"].call[c["rows"].has_row], minlength=3)
        print(f"ambient-aware calls: {n[CALL_SNG]} SNG, {n[CALL_DBL]} DBL, {n[CALL_AMB]} AMB", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
