"""Host-side mirror of the reference's interface for the likelihood path, over the C-ABI (demuxlet_amd/capi.py).

Names follow the reference: `Store` is sc_dropseq_lib_t (add_snp/add_cell/add_read, sc_drop_seq.h:34-58); `Engine` runs what
cmd_cram_demuxlet.cpp:390-734 computes; `write_single` / `write_doublet` are the writers of :465-527 and :713-875.
Everything numerical happens in libdmx.so (HIP); this module only owns buffers and marshals pointers."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import capi
from .capi import check


def device_warm_up(device: int = 0, n_gpus: int = 1) -> None:
    """dmx_device_warm_up: HIP context(s) and this library's code object, ahead of the first job of the process."""
    check(capi.load().dmx_device_warm_up(int(device), int(n_gpus)))


def phred_tables():
    mat, err = np.zeros(256), np.zeros(256)
    check(capi.load().dmx_phred_tables(mat.ctypes.data, err.ctypes.data))
    return mat, err


def geno_from_gt(alleles, gt_error: float) -> np.ndarray:
    a = np.ascontiguousarray(alleles, dtype=np.int32).reshape(-1, 2)
    out = np.zeros((a.shape[0], 3), dtype=np.float32)
    check(capi.load().dmx_geno_from_gt(a.ctypes.data, a.shape[0], gt_error, out.ctypes.data))
    return out


def geno_from_pl(pl) -> np.ndarray:
    a = np.ascontiguousarray(pl, dtype=np.int32).reshape(-1, 3)
    out = np.zeros((a.shape[0], 3), dtype=np.float32)
    check(capi.load().dmx_geno_from_pl(a.ctypes.data, a.shape[0], out.ctypes.data))
    return out


def geno_from_gp(gp, gt_error: float) -> np.ndarray:
    a = np.ascontiguousarray(gp, dtype=np.float32).reshape(-1, 3)
    out = np.zeros((a.shape[0], 3), dtype=np.float32)
    check(capi.load().dmx_geno_from_gp(a.ctypes.data, a.shape[0], gt_error, out.ctypes.data))
    return out


@dataclass
class HostPileup:
    """numpy view of a dmx_pileup in host memory (arrays are kept alive by this object)."""
    n_cells: int
    n_snps: int
    cell_pair_off: np.ndarray
    cell_read_off: np.ndarray
    pair_snp: Optional[np.ndarray]
    pair_nrd: np.ndarray
    reads: np.ndarray
    rd_totl: np.ndarray
    rd_pass: np.ndarray
    rd_uniq: np.ndarray

    def as_struct(self) -> capi.Pileup:
        for name, dt in (("cell_pair_off", np.int64), ("cell_read_off", np.int64), ("reads", np.uint8),
                         ("rd_totl", np.int32), ("rd_pass", np.int32), ("rd_uniq", np.int32)):
            setattr(self, name, np.ascontiguousarray(getattr(self, name), dtype=dt))
        if self.pair_snp is not None:
            self.pair_snp = np.ascontiguousarray(self.pair_snp, dtype=np.int32)
        if self.pair_nrd.dtype not in (np.uint8, np.uint16, np.uint32):
            self.pair_nrd = self.pair_nrd.astype(np.uint32)
        self.pair_nrd = np.ascontiguousarray(self.pair_nrd)
        return capi.Pileup(self.n_cells, self.n_snps, len(self.pair_nrd), len(self.reads),
                           self.cell_pair_off.ctypes.data, self.cell_read_off.ctypes.data,
                           self.pair_snp.ctypes.data if self.pair_snp is not None else None,
                           self.pair_nrd.ctypes.data, self.pair_nrd.dtype.itemsize, capi.DMX_MEM_HOST,
                           self.reads.ctypes.data, self.rd_totl.ctypes.data, self.rd_pass.ctypes.data,
                           self.rd_uniq.ctypes.data)

    @property
    def n_snp_per_cell(self) -> np.ndarray:
        return np.diff(self.cell_pair_off).astype(np.int32)


class Store:
    """sc_dropseq_lib_t (sc_drop_seq.h:34-58): the UMI-deduplicated pileup, built read by read."""

    def __init__(self):
        self._L = capi.load()
        self._h = self._L.dmx_store_new()
        if not self._h:
            check(-6)

    def close(self):
        if self._h:
            self._L.dmx_store_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def handle(self):
        return self._h

    def add_snp(self) -> int: return check(self._L.dmx_store_add_snp(self._h))
    def add_cell(self, barcode: str) -> int: return check(self._L.dmx_store_add_cell(self._h, barcode.encode()))
    def count_read(self, cell: int) -> None: check(self._L.dmx_store_count_read(self._h, cell))

    def add_read(self, snp: int, cell: int, umi: str, allele: int, bq: int) -> bool:
        return bool(check(self._L.dmx_store_add_read(self._h, snp, cell, umi.encode(), allele, bq)))

    def add_batch(self, snp, cell, umis: Sequence[str], allele, bq, n_threads: int = 0) -> np.ndarray:
        """len(umis) add_read calls in order, inserted on several host threads (dmx_store_add_batch); returns their return values."""
        n = len(umis)
        snp = np.ascontiguousarray(snp, dtype=np.int32); cell = np.ascontiguousarray(cell, dtype=np.int32)
        allele = np.ascontiguousarray(allele, dtype=np.uint8); bq = np.ascontiguousarray(bq, dtype=np.uint8)
        enc = [u.encode() for u in umis]
        lens = np.array([len(b) for b in enc], dtype=np.uint32)
        offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64) if n else np.zeros(0, np.uint64)
        pool = b"".join(enc) + b"\0"
        new = np.zeros(n, dtype=np.uint8)
        check(self._L.dmx_store_add_batch(self._h, n, snp.ctypes.data, cell.ctypes.data, pool, offs.ctypes.data, lens.ctypes.data,
                                          allele.ctypes.data, bq.ctypes.data, new.ctypes.data, n_threads))
        return new

    @property
    def n_cells(self) -> int: return self._L.dmx_store_n_cells(self._h)
    @property
    def n_snps(self) -> int: return self._L.dmx_store_n_snps(self._h)

    def barcodes(self) -> List[str]:
        return [self._L.dmx_store_barcode(self._h, i).decode() for i in range(self.n_cells)]

    def freeze(self) -> HostPileup:
        pl = capi.Pileup()
        check(self._L.dmx_store_freeze(self._h, C.byref(pl)))

        def arr(ptr, n, dt):
            if n == 0 or not ptr:
                return np.zeros(0, dtype=dt)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,)).copy()

        nrd_dt = {1: np.uint8, 2: np.uint16, 4: np.uint32}[pl.nrd_width]
        B = pl.n_cells
        return HostPileup(B, pl.n_snps, arr(pl.cell_pair_off, B + 1, np.int64), arr(pl.cell_read_off, B + 1, np.int64),
                          arr(pl.pair_snp, pl.n_pairs, np.int32), arr(pl.pair_nrd, pl.n_pairs, nrd_dt),
                          arr(pl.reads, pl.n_reads, np.uint8), arr(pl.rd_totl, B, np.int32), arr(pl.rd_pass, B, np.int32),
                          arr(pl.rd_uniq, B, np.int32))


class Engine:
    """The likelihood engine on one MI355X."""

    def __init__(self, n_samples: int, alphas: Sequence[float] = (0.0, 0.5), doublet_prior: float = 0.5, device: int = 0,
                 mode: int = capi.DMX_MODE_STRICT, flags: int = 0):
        self._L = capi.load()
        self.V = int(n_samples)
        self.alphas = np.ascontiguousarray(alphas, dtype=np.float64)
        self.A = len(self.alphas)
        self.prior = float(doublet_prior)
        cfg = capi.EngineConfig(self.V, self.A, self.alphas.ctypes.data, self.prior, device, mode, flags)
        h = C.c_void_p()
        check(self._L.dmx_engine_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self._keep = []
        self.B = 0
        self.S = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.dmx_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def set_stream(self, hip_stream: int) -> None:
        check(self._L.dmx_engine_set_stream(self._h, C.c_void_p(hip_stream)))

    def set_phred_tables(self, mat: np.ndarray, err: np.ndarray) -> None:
        """dmx_engine_set_phred_tables: the engine's own match / error tables (256 doubles each) instead of PhredHelper's."""
        m = np.ascontiguousarray(mat, dtype=np.float64); e = np.ascontiguousarray(err, dtype=np.float64)
        assert m.shape == (256,) and e.shape == (256,)
        check(self._L.dmx_engine_set_phred_tables(self._h, m.ctypes.data, e.ctypes.data))

    def set_genotypes(self, g: np.ndarray) -> None:
        g = np.ascontiguousarray(g, dtype=np.float32)
        if g.ndim != 3 or g.shape[1] != self.V or g.shape[2] != 3:
            raise ValueError(f"g must be [S][{self.V}][3]")
        check(self._L.dmx_engine_set_genotypes(self._h, g.ctypes.data, g.shape[0], capi.DMX_MEM_HOST))
        self._g_snps = g.shape[0]

    def set_genotypes_device(self, ptr: int, n_snps: int) -> None:
        check(self._L.dmx_engine_set_genotypes(self._h, C.c_void_p(ptr), n_snps, capi.DMX_MEM_DEVICE))
        self._g_snps = int(n_snps)

    def set_pileup(self, pl: HostPileup) -> None:
        st = pl.as_struct()
        self._keep = [pl]
        check(self._L.dmx_engine_set_pileup(self._h, C.byref(st)))
        self.B = pl.n_cells
        self.S = pl.n_snps

    def set_pileup_struct(self, st: capi.Pileup, keep=None) -> None:
        self._keep = [keep]
        check(self._L.dmx_engine_set_pileup(self._h, C.byref(st)))
        self.B = st.n_cells
        self.S = st.n_snps

    def run_singlet(self) -> None: check(self._L.dmx_engine_run_singlet(self._h))
    def run_doublet(self) -> None: check(self._L.dmx_engine_run_doublet(self._h))
    def run(self) -> None: check(self._L.dmx_engine_run(self._h))   # K1 beside K2 -> K3 -> K3b (dmx_engine_run)
    def sync(self) -> None: check(self._L.dmx_engine_sync(self._h))

    def get_singlet(self):
        llks = np.zeros((self.B, self.V))
        llk0s = np.zeros(self.B)
        check(self._L.dmx_engine_get_singlet(self._h, llks.ctypes.data, llk0s.ctypes.data))
        return llks, llk0s

    def get_doublet(self, want_grid: bool = True):
        grid = np.zeros((self.B, self.V, self.V, self.A)) if want_grid else None
        l00 = np.zeros((self.B, self.A))
        summ = np.zeros(self.B, dtype=capi.SUMMARY_DTYPE)
        check(self._L.dmx_engine_get_doublet(self._h, grid.ctypes.data if want_grid else None, l00.ctypes.data,
                                             summ.ctypes.data))
        return grid, l00, summ

    def get_sing(self) -> np.ndarray:
        sing = np.zeros((self.B, self.V))
        check(self._L.dmx_engine_get_sing(self._h, sing.ctypes.data))
        return sing

    def get_cell_grids(self, cells) -> np.ndarray:
        """llksAB[V][V][A] of the given cells (dmx_engine_get_cell_grids): the grids of the barcodes K3 flagged as near-ties are what a
        records-only consumer (write_doublet_summary, the multi-GPU gather) needs besides the records."""
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        out = np.zeros((len(cells), self.V, self.V, self.A), dtype=np.float64)
        check(self._L.dmx_engine_get_cell_grids(self._h, cells.ctypes.data, len(cells), out.ctypes.data))
        return out

    def format_pair(self, cells, barcodes: Sequence[str], sample_ids: Sequence[str], host_rows=None, ovr=None, scalars=False):
        """dmx_engine_format_pair: the `.pair` rows (cmd_cram_demuxlet.cpp:772-797) of the barcodes `cells` (ids of the staged pileup, output order) formatted on
        the device.  Returns (text bytes, cell_off[n+1], cell_flag[n], patches as a list of (offset, value, out_cell, singlet), format_ms): the POSTPRB fields the
        device leaves to the host's libm are EMPTY in the text and listed in `patches`.  With scalars=True a sixth item follows: per OUTPUT barcode the
        (max_llk, sum_single, sum_double) the text was printed from and a patch is computed from (dmx_pair_text_get_scalars: K3's record, or the
        certified grid's where `ovr` changes the grid), a structured array [n]."""
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        n = len(cells)
        bc, k1 = _cstrs(barcodes)
        sm, k2 = _cstrs(sample_ids)
        hr = np.ascontiguousarray(host_rows, dtype=np.uint8) if host_rows is not None else None
        ov = None
        if ovr is not None:
            ov = (capi.PairOverride * max(n, 1))()
            for i, o in enumerate(ovr):
                ov[i] = capi.PairOverride(*o) if o is not None else capi.PairOverride(-1, -1, -1, 0, 0.0, 0.0)
        rq = capi.PairRequest(n, cells.ctypes.data if n else None, C.cast(bc, C.c_void_p), C.cast(sm, C.c_void_p),
                              hr.ctypes.data if hr is not None else None, C.cast(ov, C.c_void_p) if ov is not None else None)
        h = C.c_void_p()
        check(self._L.dmx_engine_format_pair(self._h, C.byref(rq), C.byref(h)))
        try:
            info = capi.PairTextInfo()
            check(self._L.dmx_pair_text_get_info(h, C.byref(info)))
            buf = C.create_string_buffer(max(int(info.n_bytes), 1))
            check(self._L.dmx_pair_text_read(h, 0, info.n_bytes, buf))
            off = np.array([info.cell_off[i] for i in range(n + 1)], dtype=np.int64)
            flag = np.array([info.cell_flag[i] for i in range(n)], dtype=np.uint8)
            patches = [(int(info.patches[i].offset), float(info.patches[i].value), int(info.patches[i].out_cell), int(info.patches[i].singlet))
                       for i in range(info.n_patches)]
            if not scalars:
                return buf.raw[:info.n_bytes], off, flag, patches, float(info.format_ms)
            sp = C.POINTER(capi.PairScalars)()
            check(self._L.dmx_pair_text_get_scalars(h, C.byref(sp)))
            sc = np.zeros(n, dtype=[("max_llk", np.float64), ("sum_single", np.float64), ("sum_double", np.float64)])
            for i in range(n):
                sc[i] = (sp[i].max_llk, sp[i].sum_single, sp[i].sum_double)
            return buf.raw[:info.n_bytes], off, flag, patches, float(info.format_ms), sc
        finally:
            self._L.dmx_pair_text_free(h)

    def refine_genotypes(self, assign, prior: np.ndarray, floor: float = 1e-3):
        """dmx_engine_refine_genotypes over the staged pileup: pooled per-sample genotype likelihoods of the barcodes assign[b] = sample
        (-1 = not used) and the refined matrix.  `assign` is a host array, or a device pointer (int) to B int32.  Returns
        (LL[S][V][3] f64, n_cell[S][V], n_ref[S][V], n_alt[S][V] i32, gp'[S][V][3] f32)."""
        prior = np.ascontiguousarray(prior, dtype=np.float32)
        if prior.ndim != 3 or prior.shape[1] != self.V or prior.shape[2] != 3:
            raise ValueError(f"prior must be [S][{self.V}][3]")
        if isinstance(assign, int):
            a, mem, ptr = None, capi.DMX_MEM_DEVICE, assign
        else:
            a = np.ascontiguousarray(assign, dtype=np.int32)
            mem, ptr = capi.DMX_MEM_HOST, (a.ctypes.data if a.size else None)
        S = prior.shape[0]
        rq = capi.RefineRequest(self.B, mem, ptr, S, 0, prior.ctypes.data if prior.size else None, float(floor))
        check(self._L.dmx_engine_refine_genotypes(self._h, C.byref(rq)))
        ll = np.zeros((S, self.V, 3))
        n_cell, n_ref, n_alt = (np.zeros((S, self.V), dtype=np.int32) for _ in range(3))
        gp = np.zeros((S, self.V, 3), dtype=np.float32)
        check(self._L.dmx_engine_get_refined(self._h, ll.ctypes.data, n_cell.ctypes.data, n_ref.ctypes.data, n_alt.ctypes.data, gp.ctypes.data))
        return ll, n_cell, n_ref, n_alt, gp

    def refined_device_ptr(self) -> int:
        """Device pointer of the last refined matrix gp' [S][V][3] f32 (for set_genotypes_device)."""
        p = C.c_void_p()
        check(self._L.dmx_engine_refined_device_ptr(self._h, C.byref(p)))
        return int(p.value)

    def refine_info(self) -> dict:
        """HIP-event times (ms) and sizes of the last refinement (dmx_engine_refine_info)."""
        r = capi.RefineInfo()
        check(self._L.dmx_engine_refine_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.RefineInfo._fields_ if n != "reserved"}

    def cluster_stage(self) -> None:
        """dmx_engine_cluster_stage: the SNP-major cache of the staged pileup (per-pair log GL, REF / ALT reads, cell ids)."""
        check(self._L.dmx_engine_cluster_stage(self._h))

    def get_cluster_stage(self):
        """The stage cache: (snp_off[S + 1] i64, cell[P] i32, lgl[P][3] f64, n_ref[P], n_alt[P] i64)."""
        inf = self.cluster_info()
        S, P = inf["n_snps"], inf["n_pairs"]
        off = np.zeros(S + 1, dtype=np.int64)
        cell = np.zeros(P, dtype=np.int32)
        lgl = np.zeros((P, 3))
        ra = np.zeros(P, dtype=np.uint32)
        check(self._L.dmx_engine_get_cluster_stage(self._h, off.ctypes.data, cell.ctypes.data, lgl.ctypes.data, ra.ctypes.data))
        return off, cell, lgl, (ra & 0xFFFF).astype(np.int64), (ra >> 16).astype(np.int64)

    def cluster_mstep(self, weights, prior: np.ndarray, floor: float = 1e-3, fetch: bool = True):
        """dmx_engine_cluster_mstep: weights is a host array [B][V] f64, a device pointer (int), or None = the last E-step's; prior [S][3].
        Returns (LL[S][V][3] f64, W[S][V] f64, gp'[S][V][3] f32), or None with fetch=False (gp' stays on the device: cluster_device_ptr)."""
        prior = np.ascontiguousarray(prior, dtype=np.float32)
        if prior.ndim != 2 or prior.shape[1] != 3:
            raise ValueError("prior must be [S][3]")
        S = prior.shape[0]
        w = None
        if weights is None:
            mem, ptr = capi.DMX_CLUSTER_LAST_ESTEP, None
        elif isinstance(weights, int):
            mem, ptr = capi.DMX_MEM_DEVICE, weights
        else:
            w = np.ascontiguousarray(weights, dtype=np.float64)
            if w.shape != (self.B, self.V):
                raise ValueError(f"weights must be [{self.B}][{self.V}]")
            mem, ptr = capi.DMX_MEM_HOST, (w.ctypes.data if w.size else None)
        rq = capi.ClusterMstepRequest(self.B, S, self.V, mem, ptr, prior.ctypes.data if prior.size else None, float(floor))
        check(self._L.dmx_engine_cluster_mstep(self._h, C.byref(rq)))
        if not fetch:
            return None
        return self.get_cluster(S)

    def get_cluster(self, n_snps: int):
        ll = np.zeros((n_snps, self.V, 3))
        W = np.zeros((n_snps, self.V))
        gp = np.zeros((n_snps, self.V, 3), dtype=np.float32)
        check(self._L.dmx_engine_get_cluster(self._h, ll.ctypes.data, W.ctypes.data, gp.ctypes.data, None))
        return ll, W, gp

    def cluster_genotypes(self, n_snps: int) -> np.ndarray:
        """The last M-step's gp' [S][V][3] f32 alone."""
        gp = np.zeros((n_snps, self.V, 3), dtype=np.float32)
        check(self._L.dmx_engine_get_cluster(self._h, None, None, gp.ctypes.data, None))
        return gp

    def cluster_weights(self) -> np.ndarray:
        """The last E-step's weights [B][V] f64."""
        w = np.zeros((self.B, self.V))
        check(self._L.dmx_engine_get_cluster(self._h, None, None, None, w.ctypes.data))
        return w

    def cluster_estep(self, n_restarts: int, n_clusters: int, log_pi, temperature: float = 1.0, mask=None):
        """dmx_engine_cluster_estep on K1's llks of the last run_singlet: the weights stay on the device; returns (ll[R], col_sum[R * K])."""
        lp = np.ascontiguousarray(log_pi, dtype=np.float64).reshape(-1)
        if lp.size != n_restarts * n_clusters:
            raise ValueError("log_pi must be [R][K]")
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        if m is not None and m.shape != (self.B,):
            raise ValueError(f"mask must be [{self.B}]")
        ll = np.zeros(n_restarts)
        cs = np.zeros(n_restarts * n_clusters)
        rq = capi.ClusterEstepRequest(int(n_restarts), int(n_clusters), lp.ctypes.data, float(temperature), m.ctypes.data if m is not None and m.size else None,
                                      ll.ctypes.data, cs.ctypes.data)
        check(self._L.dmx_engine_cluster_estep(self._h, C.byref(rq)))
        return ll, cs

    def cluster_device_ptr(self) -> int:
        """Device pointer of the last M-step's gp' [S][V][3] f32 (for set_genotypes_device)."""
        p = C.c_void_p()
        check(self._L.dmx_engine_cluster_device_ptr(self._h, C.byref(p)))
        return int(p.value)

    def cluster_info(self) -> dict:
        """HIP-event times (ms) of the last stage / M-step / E-step and the cache's size (dmx_engine_cluster_info)."""
        r = capi.ClusterInfo()
        check(self._L.dmx_engine_cluster_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.ClusterInfo._fields_ if n != "reserved"}

    def cluster_doublet(self, n_restarts: int, n_clusters: int) -> None:
        """dmx_engine_cluster_doublet: LLD[B][R][P] of the pairs k < l of clusters within each restart (alpha = 0.5), kept on the device."""
        check(self._L.dmx_engine_cluster_doublet(self._h, int(n_restarts), int(n_clusters)))

    def get_cluster_doublet(self):
        """The last (LLD [B][R][P] f64, pairs (k, l), k < l, in lexicographic order; lsc [B] f64, the scale term: LLD - lsc is on K1's scale)."""
        inf = self.cluster_doublet_info()
        lld = np.zeros((inf["n_cells"], inf["n_restarts"], inf["n_pairs"]))
        lsc = np.zeros(inf["n_cells"])
        check(self._L.dmx_engine_get_cluster_doublet(self._h, lld.ctypes.data if lld.size else None, lsc.ctypes.data if lsc.size else None))
        return lld, lsc

    def cluster_doublet_scale(self) -> np.ndarray:
        """lsc [B] f64 of the last cluster_doublet alone (LLD stays on the device): LLD - lsc is on K1's scale."""
        lsc = np.zeros(self.cluster_doublet_info()["n_cells"])
        check(self._L.dmx_engine_get_cluster_doublet(self._h, None, lsc.ctypes.data if lsc.size else None))
        return lsc

    def cluster_estep_doublet(self, n_restarts: int, n_clusters: int, log_pi, log_delta, temperature: float = 1.0, mask=None):
        """dmx_engine_cluster_estep_doublet on K1's llks of the last run_singlet and the last LLD: the singlet weights stay on the device;
        returns (ll[R], col_sum[R * K], dbl_mass[R])."""
        lp = np.ascontiguousarray(log_pi, dtype=np.float64).reshape(-1)
        ld = np.ascontiguousarray(log_delta, dtype=np.float64).reshape(-1)
        if lp.size != n_restarts * n_clusters:
            raise ValueError("log_pi must be [R][K]")
        if ld.size != n_restarts:
            raise ValueError("log_delta must be [R]")
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        if m is not None and m.shape != (self.B,):
            raise ValueError(f"mask must be [{self.B}]")
        ll = np.zeros(n_restarts)
        cs = np.zeros(n_restarts * n_clusters)
        dm = np.zeros(n_restarts)
        rq = capi.ClusterEstepDoubletRequest(int(n_restarts), int(n_clusters), lp.ctypes.data, ld.ctypes.data, float(temperature),
                                             m.ctypes.data if m is not None and m.size else None, ll.ctypes.data, cs.ctypes.data, dm.ctypes.data)
        check(self._L.dmx_engine_cluster_estep_doublet(self._h, C.byref(rq)))
        return ll, cs, dm

    def cluster_doublet_info(self) -> dict:
        """HIP-event times (ms) of the last doublet likelihoods / doublet E-step and LLD's size (dmx_engine_cluster_doublet_info)."""
        r = capi.ClusterDoubletInfo()
        check(self._L.dmx_engine_cluster_doublet_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.ClusterDoubletInfo._fields_ if n != "reserved"}

    def cluster_merge_score(self, n_restarts: int, n_clusters: int, prior: np.ndarray, floor: float = 1e-3):
        """dmx_engine_cluster_merge_score on the last M-step: (bf[R][P] f64, n_shared[R][P] i32), pairs (k, l), k < l, lexicographic."""
        prior = np.ascontiguousarray(prior, dtype=np.float32)
        if prior.ndim != 2 or prior.shape[1] != 3:
            raise ValueError("prior must be [S][3]")
        P = n_clusters * (n_clusters - 1) // 2
        bf = np.zeros((n_restarts, P))
        ns = np.zeros((n_restarts, P), dtype=np.int32)
        check(self._L.dmx_engine_cluster_merge_score(self._h, int(n_restarts), int(n_clusters), prior.ctypes.data if prior.size else None,
                                                     float(floor), bf.ctypes.data if bf.size else None, ns.ctypes.data if ns.size else None))
        return bf, ns

    def cluster_estep_grouped(self, n_restarts: int, n_clusters: int, log_pi, group, restarts_per_group: int, temperature: float = 1.0, mask=None):
        """dmx_engine_cluster_estep_grouped: restart r sees only the barcodes with group[b] == r // restarts_per_group; the weights stay on
        the device; returns (ll[R], col_sum[R * K])."""
        lp = np.ascontiguousarray(log_pi, dtype=np.float64).reshape(-1)
        if lp.size != n_restarts * n_clusters:
            raise ValueError("log_pi must be [R][K]")
        grp = np.ascontiguousarray(group, dtype=np.int32)
        if grp.shape != (self.B,):
            raise ValueError(f"group must be [{self.B}]")
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        if m is not None and m.shape != (self.B,):
            raise ValueError(f"mask must be [{self.B}]")
        ll = np.zeros(n_restarts)
        cs = np.zeros(n_restarts * n_clusters)
        rq = capi.ClusterEstepGroupedRequest(int(n_restarts), int(n_clusters), lp.ctypes.data, float(temperature),
                                             m.ctypes.data if m is not None and m.size else None, grp.ctypes.data if grp.size else None,
                                             int(restarts_per_group), 0, ll.ctypes.data, cs.ctypes.data)
        check(self._L.dmx_engine_cluster_estep_grouped(self._h, C.byref(rq)))
        return ll, cs

    def cluster_sm_info(self) -> dict:
        """HIP-event times (ms) of the last merge score / grouped E-step (dmx_engine_cluster_sm_info)."""
        r = capi.ClusterSmInfo()
        check(self._L.dmx_engine_cluster_sm_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.ClusterSmInfo._fields_ if n != "reserved"}

    def cluster_evidence(self, n_restarts: int, n_clusters: int, prior: np.ndarray, floor: float = 1e-3):
        """dmx_engine_cluster_evidence on the last M-step: (ev[R][K] f64, the log marginal likelihood of each column's reads with the
        genotypes integrated out; n_cov[R][K] i32, its covered SNPs)."""
        prior = np.ascontiguousarray(prior, dtype=np.float32)
        if prior.ndim != 2 or prior.shape[1] != 3:
            raise ValueError("prior must be [S][3]")
        ev = np.zeros((max(int(n_restarts), 0), max(int(n_clusters), 0)))
        nc = np.zeros(ev.shape, dtype=np.int32)
        check(self._L.dmx_engine_cluster_evidence(self._h, int(n_restarts), int(n_clusters), prior.ctypes.data if prior.size else None,
                                                  float(floor), ev.ctypes.data if ev.size else None, nc.ctypes.data if nc.size else None))
        return ev, nc

    def cluster_hard(self, n_restarts: int, n_clusters: int, active, mask=None, doublets: bool = False):
        """dmx_engine_cluster_hard on the last E-step's weights: active [R][K] (1 = the column takes part).  Returns (label[B][R] i32: the
        cluster, -1 outside the mask, -2 - p for a doublet of pair p; n_sing[R][K] i32; n_dbl[R] i32; dbl_score[R] f64).  The one-hot
        matrix of the singlet labels stays on the device (cluster_hard_device_ptr)."""
        R, K = int(n_restarts), int(n_clusters)
        act = np.ascontiguousarray(active, dtype=np.uint8).reshape(-1)
        if act.size != max(R, 0) * max(K, 0):
            raise ValueError("active must be [R][K]")
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        if m is not None and m.shape != (self.B,):
            raise ValueError(f"mask must be [{self.B}]")
        label = np.zeros((self.B, max(R, 0)), dtype=np.int32)
        n_sing = np.zeros((max(R, 0), max(K, 0)), dtype=np.int32)
        n_dbl = np.zeros(max(R, 0), dtype=np.int32)
        score = np.zeros(max(R, 0))
        rq = capi.ClusterHardRequest(R, K, int(bool(doublets)), 0, act.ctypes.data if act.size else None,
                                     m.ctypes.data if m is not None and m.size else None, label.ctypes.data if label.size else None,
                                     n_sing.ctypes.data if n_sing.size else None, n_dbl.ctypes.data if n_dbl.size else None,
                                     score.ctypes.data if score.size else None)
        check(self._L.dmx_engine_cluster_hard(self._h, C.byref(rq)))
        return label, n_sing, n_dbl, score

    def get_cluster_hard(self, n_restarts: int, n_clusters: int, dbl_mass: bool = False):
        """The last hard labels' device results: (label[B][R] i32, score[B][R] f64: each barcode's doublet score, hot[B][R * K] f64: the
        one-hot matrix) and, with dbl_mass, the doublet mass [B][R] f64 they were made from."""
        label = np.zeros((self.B, n_restarts), dtype=np.int32)
        score = np.zeros((self.B, n_restarts))
        hot = np.zeros((self.B, n_restarts * n_clusters))
        dm = np.zeros((self.B, n_restarts)) if dbl_mass else None
        check(self._L.dmx_engine_get_cluster_hard(self._h, label.ctypes.data, score.ctypes.data, hot.ctypes.data, dm.ctypes.data if dbl_mass else None))
        return (label, score, hot, dm) if dbl_mass else (label, score, hot)

    def cluster_hard_device_ptr(self) -> int:
        """Device pointer of the last one-hot matrix [B][R * K] f64 (for cluster_mstep(weights=<int>))."""
        p = C.c_void_p()
        check(self._L.dmx_engine_cluster_hard_device_ptr(self._h, C.byref(p)))
        return int(p.value)

    def cluster_merge_columns(self, n_restarts: int, n_clusters: int, merge_from, merge_into) -> None:
        """dmx_engine_cluster_merge_columns: in every restart r with merge_from[r] >= 0 the last E-step's weights of column merge_from[r]
        are added to column merge_into[r] and zeroed, on the device (the next cluster_mstep(None, ...) reads them)."""
        f = np.ascontiguousarray(merge_from, dtype=np.int32).reshape(-1)
        t = np.ascontiguousarray(merge_into, dtype=np.int32).reshape(-1)
        if f.size != n_restarts or t.size != n_restarts:
            raise ValueError("merge_from and merge_into must be [R]")
        check(self._L.dmx_engine_cluster_merge_columns(self._h, int(n_restarts), int(n_clusters), f.ctypes.data if f.size else None,
                                                       t.ctypes.data if t.size else None))

    def cluster_k_info(self) -> dict:
        """HIP-event times (ms) of the last evidence / hard labels / column merge (dmx_engine_cluster_k_info)."""
        r = capi.ClusterKInfo()
        check(self._L.dmx_engine_cluster_k_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.ClusterKInfo._fields_ if n != "reserved"}

    def cluster_set_known(self, g) -> None:
        """dmx_engine_cluster_set_known: the known rows [S][Vk][3] f32 (a host array) shared by every restart of the windowed M-step."""
        g = np.ascontiguousarray(g, dtype=np.float32)
        if g.ndim != 3 or g.shape[2] != 3:
            raise ValueError("known rows must be [S][Vk][3]")
        check(self._L.dmx_engine_cluster_set_known(self._h, g.shape[0], g.shape[1], g.ctypes.data if g.size else None, capi.DMX_MEM_HOST))

    def cluster_estep_known(self, n_restarts: int, n_known: int, n_free: int, log_pi, temperature: float = 1.0, mask=None):
        """dmx_engine_cluster_estep_known on K1's llks of the last run_singlet, columns [Vk known | R x M free]: the free weights
        [B][R * M] stay on the device; returns (ll[R], col_sum[R][Vk + M])."""
        R, K = int(n_restarts), int(n_known) + int(n_free)
        lp = np.ascontiguousarray(log_pi, dtype=np.float64).reshape(-1)
        if lp.size != R * K:
            raise ValueError("log_pi must be [R][Vk + M]")
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        if m is not None and m.shape != (self.B,):
            raise ValueError(f"mask must be [{self.B}]")
        ll = np.zeros(R)
        cs = np.zeros((R, K))
        rq = capi.ClusterEstepKnownRequest(R, int(n_known), int(n_free), 0, lp.ctypes.data, float(temperature),
                                           m.ctypes.data if m is not None and m.size else None, ll.ctypes.data, cs.ctypes.data)
        check(self._L.dmx_engine_cluster_estep_known(self._h, C.byref(rq)))
        return ll, cs

    def cluster_mstep_window(self, weights, n_restarts: int, n_free: int, prior: np.ndarray, floor: float = 1e-3, fetch: bool = True):
        """dmx_engine_cluster_mstep_window over the R * M free columns: weights is a host array [B][R * M] f64, a device pointer (int), or
        None = the last known-column E-step's; prior [S][3].  Returns (LL[S][R * M][3] f64, W[S][R * M] f64, gp'[S][V][3] f32, whose
        first Vk columns are the known rows), or None with fetch=False (gp' stays on the device: cluster_device_ptr)."""
        prior = np.ascontiguousarray(prior, dtype=np.float32)
        if prior.ndim != 2 or prior.shape[1] != 3:
            raise ValueError("prior must be [S][3]")
        S, CF = prior.shape[0], int(n_restarts) * int(n_free)
        w = None
        if weights is None:
            mem, ptr = capi.DMX_CLUSTER_LAST_ESTEP, None
        elif isinstance(weights, int):
            mem, ptr = capi.DMX_MEM_DEVICE, weights
        else:
            w = np.ascontiguousarray(weights, dtype=np.float64)
            if w.shape != (self.B, CF):
                raise ValueError(f"weights must be [{self.B}][{CF}]")
            mem, ptr = capi.DMX_MEM_HOST, (w.ctypes.data if w.size else None)
        rq = capi.ClusterMstepWindowRequest(self.B, S, int(n_restarts), int(n_free), mem, 0, ptr, prior.ctypes.data if prior.size else None,
                                            float(floor))
        check(self._L.dmx_engine_cluster_mstep_window(self._h, C.byref(rq)))
        if not fetch:
            return None
        ll = np.zeros((S, CF, 3))
        W = np.zeros((S, CF))
        gp = np.zeros((S, self.V, 3), dtype=np.float32)
        check(self._L.dmx_engine_get_cluster(self._h, ll.ctypes.data, W.ctypes.data, gp.ctypes.data, None))
        return ll, W, gp

    def cluster_known_weights(self):
        """(every component's weights [B][R][Vk + M], the free weights [B][R * M]) of the last known-column E-step."""
        inf = self.cluster_known_info()
        B, R, Vk, M = inf["n_cells"], inf["n_restarts"], inf["n_known"], inf["n_free"]
        wk = np.zeros((B, R, Vk + M))
        wf = np.zeros((B, R * M))
        check(self._L.dmx_engine_get_cluster_known(self._h, wk.ctypes.data))
        check(self._L.dmx_engine_get_cluster(self._h, None, None, None, wf.ctypes.data))
        return wk, wf

    def cluster_known_info(self) -> dict:
        """HIP-event times (ms) of the last known-column E-step / windowed M-step (dmx_engine_cluster_known_info)."""
        r = capi.ClusterKnownInfo()
        check(self._L.dmx_engine_cluster_known_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.ClusterKnownInfo._fields_ if n != "reserved"}

    def ambient_profile(self, assign, ambient, grid):
        """dmx_engine_ambient over the staged pileup: LL[b][q] of each barcode assigned to sample assign[b] (-1 = not used) with a fraction
        grid[q] of its reads from a soup of ALT frequency ambient[i].  `assign` is a host array, or a device pointer (int) to B int32.
        Returns (ll[B][Q] f64, n_snp[B] i32, n_read[B] i32)."""
        amb = np.ascontiguousarray(ambient, dtype=np.float64)
        gr = np.ascontiguousarray(grid, dtype=np.float64)
        if amb.ndim != 1 or gr.ndim != 1:
            raise ValueError("ambient and grid must be 1-D")
        if isinstance(assign, int):
            a, mem, ptr = None, capi.DMX_MEM_DEVICE, assign
        else:
            a = np.ascontiguousarray(assign, dtype=np.int32)
            if a.shape != (self.B,):
                raise ValueError(f"assign must be [{self.B}]")
            mem, ptr = capi.DMX_MEM_HOST, (a.ctypes.data if a.size else None)
        Q = len(gr)
        rq = capi.AmbientRequest(self.B, mem, ptr, len(amb), Q, amb.ctypes.data if amb.size else None, gr.ctypes.data if gr.size else None)
        check(self._L.dmx_engine_ambient(self._h, C.byref(rq)))
        ll = np.zeros((self.B, Q))
        n_snp = np.zeros(self.B, dtype=np.int32)
        n_read = np.zeros(self.B, dtype=np.int32)
        check(self._L.dmx_engine_get_ambient(self._h, ll.ctypes.data, n_snp.ctypes.data, n_read.ctypes.data))
        return ll, n_snp, n_read

    def ambient_info(self) -> dict:
        """HIP-event time (ms) of the last ambient profile and the profile's size (dmx_engine_ambient_info)."""
        r = capi.AmbientInfo()
        check(self._L.dmx_engine_ambient_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.AmbientInfo._fields_ if n != "reserved"}

    def ambient_doublet_profile(self, cand, alphas, ambient, grid, n_cand=None):
        """dmx_engine_ambient_doublet over the staged pileup: LL[b][c][n][q] of barcode b as a doublet of the samples cand[b][c] = (v1, v2)
        (v1 = -1: slot not used), v2 contributing a share alphas[n] of the cell's reads, with a fraction grid[q] of all reads from a soup of
        ALT frequency ambient[i].  `cand` is a host array [B][C][2], or a device pointer (int) to B x n_cand x 2 int32.
        Returns (ll[B][C][A][Q] f64, n_snp[B][C] i32, n_read[B][C] i32)."""
        amb = np.ascontiguousarray(ambient, dtype=np.float64)
        gr = np.ascontiguousarray(grid, dtype=np.float64)
        al = np.ascontiguousarray(alphas, dtype=np.float64)
        if amb.ndim != 1 or gr.ndim != 1 or al.ndim != 1:
            raise ValueError("alphas, ambient and grid must be 1-D")
        if isinstance(cand, int):
            if n_cand is None:
                raise ValueError("a device cand needs n_cand=")
            cd, mem, ptr, Cn = None, capi.DMX_MEM_DEVICE, cand, int(n_cand)
        else:
            cd = np.ascontiguousarray(cand, dtype=np.int32)
            if cd.ndim != 3 or cd.shape[0] != self.B or cd.shape[2] != 2:
                raise ValueError(f"cand must be [{self.B}][C][2]")
            mem, ptr, Cn = capi.DMX_MEM_HOST, (cd.ctypes.data if cd.size else None), cd.shape[1]
        A, Q = len(al), len(gr)
        rq = capi.AmbientDoubletRequest(self.B, mem, ptr, Cn, A, len(amb), Q, al.ctypes.data if al.size else None,
                                        amb.ctypes.data if amb.size else None, gr.ctypes.data if gr.size else None)
        check(self._L.dmx_engine_ambient_doublet(self._h, C.byref(rq)))
        ll = np.zeros((self.B, Cn, A, Q))
        n_snp = np.zeros((self.B, Cn), dtype=np.int32)
        n_read = np.zeros((self.B, Cn), dtype=np.int32)
        check(self._L.dmx_engine_get_ambient_doublet(self._h, ll.ctypes.data, n_snp.ctypes.data, n_read.ctypes.data))
        return ll, n_snp, n_read

    def ambient_doublet_info(self) -> dict:
        """HIP-event time (ms) of the last ambient-aware doublet profile and its size (dmx_engine_ambient_doublet_info)."""
        r = capi.AmbientDoubletInfo()
        check(self._L.dmx_engine_ambient_doublet_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.AmbientDoubletInfo._fields_ if n != "reserved"}

    def fit_profile(self, hyp, alpha, rho=None, ambient=None, max_reads: int = 4) -> dict:
        """dmx_engine_fit over the staged pileup: the goodness of fit of one hypothesis per barcode.  hyp[b] = (v1, v2): v1 = -1 = not used,
        v2 = -1 = a singlet of v1, otherwise a doublet with a share alpha[b] of v2's reads; rho[b] (None = 0) of the reads come from a soup
        of ALT frequency ambient[i].  `hyp` is a host array [B][2], or a device pointer (int) to B x 2 int32.  Returns a dict of obs / mean /
        var (f64 [B]: the log-likelihood of each pair's first max_reads reads, and its mean and variance under the hypothesis) and n_snp /
        n_read / n_trunc / n_zero (i32 [B])."""
        al = np.ascontiguousarray(alpha, dtype=np.float64)
        if al.shape != (self.B,):
            raise ValueError(f"alpha must be [{self.B}]")
        rh = None
        if rho is not None:
            rh = np.ascontiguousarray(rho, dtype=np.float64)
            if rh.shape != (self.B,):
                raise ValueError(f"rho must be [{self.B}]")
        amb = None
        if ambient is not None:
            amb = np.ascontiguousarray(ambient, dtype=np.float64)
            if amb.ndim != 1:
                raise ValueError("ambient must be 1-D")
        if isinstance(hyp, int):
            h, mem, ptr = None, capi.DMX_MEM_DEVICE, hyp
        else:
            h = np.ascontiguousarray(hyp, dtype=np.int32)
            if h.shape != (self.B, 2):
                raise ValueError(f"hyp must be [{self.B}][2]")
            mem, ptr = capi.DMX_MEM_HOST, (h.ctypes.data if h.size else None)
        n_snps = len(amb) if amb is not None else self.S
        rq = capi.FitRequest(self.B, n_snps, mem, int(max_reads), ptr, al.ctypes.data if al.size else None,
                             rh.ctypes.data if rh is not None and rh.size else None, amb.ctypes.data if amb is not None and amb.size else None)
        check(self._L.dmx_engine_fit(self._h, C.byref(rq)))
        out = {k: np.zeros(self.B) for k in ("obs", "mean", "var")}
        out.update({k: np.zeros(self.B, dtype=np.int32) for k in ("n_snp", "n_read", "n_trunc", "n_zero")})
        check(self._L.dmx_engine_get_fit(self._h, *(out[k].ctypes.data for k in ("obs", "mean", "var", "n_snp", "n_read", "n_trunc", "n_zero"))))
        return out

    def fit_info(self) -> dict:
        """HIP-event time (ms) of the last fit_profile, its device bytes and its totals (dmx_engine_fit_info)."""
        r = capi.FitInfo()
        check(self._L.dmx_engine_fit_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.FitInfo._fields_ if n != "reserved"}

    def site_fit(self, hyp, alpha, rho=None, ambient=None, max_reads: int = 4, partial_bytes: int = 0) -> dict:
        """dmx_engine_site_fit over the staged pileup: the goodness of fit of every SNP's row under one hypothesis per barcode (fit_profile's
        arguments).  `partial_bytes` caps the chunk-partial buffer (0 = the default budget); the results do not depend on it.  Returns a dict
        of obs / mean / var / exc / vexc (f64 [S]: fit_profile's three sums over the barcodes at the SNP, the signed excess of ALT reads over
        their expectation and its variance) and n_cell / n_read / n_alt / n_trunc / n_zero (i32 [S])."""
        al = np.ascontiguousarray(alpha, dtype=np.float64)
        if al.shape != (self.B,):
            raise ValueError(f"alpha must be [{self.B}]")
        rh, amb, n_snps = self._share_soup(rho, ambient)
        if isinstance(hyp, int):
            h, mem, ptr = None, capi.DMX_MEM_DEVICE, hyp
        else:
            h = np.ascontiguousarray(hyp, dtype=np.int32)
            if h.shape != (self.B, 2):
                raise ValueError(f"hyp must be [{self.B}][2]")
            mem, ptr = capi.DMX_MEM_HOST, (h.ctypes.data if h.size else None)
        rq = capi.SiteFitRequest(self.B, n_snps, mem, int(max_reads), ptr, al.ctypes.data if al.size else None,
                                 rh.ctypes.data if rh is not None and rh.size else None, amb.ctypes.data if amb is not None and amb.size else None,
                                 int(partial_bytes))
        check(self._L.dmx_engine_site_fit(self._h, C.byref(rq)))
        out = {k: np.zeros(n_snps) for k in ("obs", "mean", "var", "exc", "vexc")}
        out.update({k: np.zeros(n_snps, dtype=np.int32) for k in ("n_cell", "n_read", "n_alt", "n_trunc", "n_zero")})
        check(self._L.dmx_engine_get_site_fit(self._h, *(v.ctypes.data for v in out.values())))
        return out

    def site_fit_info(self) -> dict:
        """HIP-event time (ms) of the last site_fit, its device bytes, chunks, waves and totals (dmx_engine_site_fit_info)."""
        r = capi.SiteFitInfo()
        check(self._L.dmx_engine_site_fit_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.SiteFitInfo._fields_ if n != "reserved"}

    def redraw(self, hyp, alpha, rho=None, ambient=None, seed: int = 0, geno_seed: int = 0, genotype_draw: str = "donor",
               index_base: int = 0) -> dict:
        """dmx_engine_redraw over the staged pileup: every stored read of a used barcode gets a new allele drawn from fit_profile's law
        under hyp[b] (fit_profile's arguments; `hyp` a host array [B][2] or a device pointer).  genotype_draw "donor": a donor has one
        genotype per SNP in every barcode and replicate (keyed by geno_seed); "pair": a genotype per pair (keyed by seed), fit_profile's
        own law.  Barcode b is hashed as id index_base + b.  Returns the info dict (redraw_info)."""
        modes = {"pair": capi.DMX_REDRAW_PAIR, "donor": capi.DMX_REDRAW_DONOR}
        if genotype_draw not in modes:
            raise ValueError("genotype_draw must be 'donor' or 'pair'")
        al = np.ascontiguousarray(alpha, dtype=np.float64)
        if al.shape != (self.B,):
            raise ValueError(f"alpha must be [{self.B}]")
        rh, amb, n_snps = self._share_soup(rho, ambient)
        if isinstance(hyp, int):
            h, mem, ptr = None, capi.DMX_MEM_DEVICE, hyp
        else:
            h = np.ascontiguousarray(hyp, dtype=np.int32)
            if h.shape != (self.B, 2):
                raise ValueError(f"hyp must be [{self.B}][2]")
            mem, ptr = capi.DMX_MEM_HOST, (h.ctypes.data if h.size else None)
        rq = capi.RedrawRequest(self.B, n_snps, mem, modes[genotype_draw], ptr, al.ctypes.data if al.size else None,
                                rh.ctypes.data if rh is not None and rh.size else None, amb.ctypes.data if amb is not None and amb.size else None,
                                int(seed) & 0xFFFFFFFFFFFFFFFF, int(geno_seed) & 0xFFFFFFFFFFFFFFFF, int(index_base))
        check(self._L.dmx_engine_redraw(self._h, C.byref(rq)))
        return self.redraw_info()

    def redraw_info(self) -> dict:
        """HIP-event time (ms) of the last redraw's kernel, its algorithmic bytes and its counts (dmx_engine_redraw_info)."""
        r = capi.RedrawInfo()
        check(self._L.dmx_engine_redraw_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.RedrawInfo._fields_ if n != "reserved"}

    def redrawn_pileup(self) -> capi.Pileup:
        """The redrawn pileup as a device-resident dmx_pileup (dmx_engine_redrawn_pileup) for another engine's set_pileup_struct or for
        demuxlet_run: the staged source's own offsets and pair arrays with new reads; the rd_* counters are NULL (a caller that needs
        them attaches the source's host arrays).  Owned by this engine: valid until its next redraw / set_pileup / close."""
        st = capi.Pileup()
        check(self._L.dmx_engine_redrawn_pileup(self._h, C.byref(st)))
        return st

    def geno_compare(self, ga=None, gb=None, weight=None, memory: int = capi.DMX_MEM_HOST, n_snps: Optional[int] = None,
                     n_a: Optional[int] = None, n_b: Optional[int] = None):
        """dmx_engine_geno_compare: the weighted 4 x 4 joint tables of every column of ga [S][VA][3] with every column of gb [S][VB][3]
        (float32 gp-style rows), T[a][b][x][y] = sum_i weight_i ra_i[a][x] rb_i[b][y] with r = (p0, p1, p2, valid); include/dmx.h
        defines the bits.  ga = None: the engine's staged genotype matrix; gb = None: B is A; weight = None: ones.  With
        memory = DMX_MEM_DEVICE ga / gb / weight are device pointers (ints) and n_snps, n_a, n_b give the shapes.  Needs no pileup.
        Returns (table [VA][VB][4][4] float64, n_valid_a [VA] int32, n_valid_b [VB] int32)."""
        keep = []

        def side(g):
            if g is None:
                return None, None
            if memory == capi.DMX_MEM_DEVICE:
                return int(g), None
            a = np.ascontiguousarray(g, dtype=np.float32)
            if a.ndim != 3 or a.shape[2] != 3 or a.shape[1] < 1:
                raise ValueError("a genotype matrix must be [S][V][3] with V >= 1")
            keep.append(a)
            return (a.ctypes.data if a.size else None), a.shape

        pa, sa = side(ga)
        pb, sb = side(gb)
        if memory == capi.DMX_MEM_DEVICE:
            if n_snps is None or (ga is not None and n_a is None) or (gb is not None and n_b is None):
                raise ValueError("device inputs need n_snps, n_a and n_b")
            S = int(n_snps)
            VA = int(n_a) if ga is not None else self.V
            VB = int(n_b) if gb is not None else VA
            pw = int(weight) if weight is not None else None
        else:
            if sa is None and sb is None and n_snps is None:
                n_snps = getattr(self, "_g_snps", None)
                if n_snps is None:
                    raise ValueError("ga is None and no genotype matrix was staged with set_genotypes (pass n_snps)")
            S = sa[0] if sa is not None else sb[0] if sb is not None else int(n_snps)
            if sa is not None and sb is not None and sa[0] != sb[0]:
                raise ValueError(f"ga has {sa[0]} SNPs, gb has {sb[0]}")
            VA = sa[1] if sa is not None else self.V
            VB = sb[1] if sb is not None else VA
            pw = None
            if weight is not None:
                w = np.ascontiguousarray(weight, dtype=np.float64)
                if w.shape != (S,):
                    raise ValueError(f"weight must be [{S}]")
                keep.append(w)
                pw = w.ctypes.data if w.size else None
            # an empty host matrix has no address to give; the engine reads nothing at S = 0, but NULL would mean "the staged matrix"
            if ga is not None and pa is None:
                keep.append(np.zeros(4, dtype=np.float32)); pa = keep[-1].ctypes.data
            if gb is not None and pb is None:
                keep.append(np.zeros(4, dtype=np.float32)); pb = keep[-1].ctypes.data
        rq = capi.KinRequest(S, VA, VB, pa, pb, pw, memory, 0)
        check(self._L.dmx_engine_geno_compare(self._h, C.byref(rq)))
        table = np.zeros((VA, VB, 4, 4), dtype=np.float64)
        nva = np.zeros(VA, dtype=np.int32); nvb = np.zeros(VB, dtype=np.int32)
        check(self._L.dmx_engine_get_geno_compare(self._h, table.ctypes.data, nva.ctypes.data, nvb.ctypes.data))
        return table, nva, nvb

    def geno_compare_info(self) -> dict:
        """HIP-event times (ms) of the last geno_compare's two kernels, its FLOP and algorithmic bytes, the tile kernel's tile_a, tile_b
        and chunk_snps, and the invalid-row counts (dmx_engine_geno_compare_info)."""
        r = capi.KinInfo()
        check(self._L.dmx_engine_geno_compare_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.KinInfo._fields_ if n != "reserved"}

    def block_llk(self, block, n_blocks: int, extra=None, n_extra: Optional[int] = None) -> dict:
        """dmx_engine_block_llk over the staged pileup: every barcode's singlet column, llks00 and up to 8 chosen grid entries summed per
        genomic block.  block: int32 [S], non-decreasing, in [0, n_blocks).  extra: None, a host array [B][E][3] of (j, k, n) with
        j = -1 = unused, or a device pointer (int) to B x n_extra x 3 int32.  STRICT terms whatever the engine's mode; include/dmx.h
        defines the bits.  Returns col[B][G][V], l00[B][G][A], ext[B][G][E] (float64) and n_snp[B][G] (int32)."""
        blk = np.ascontiguousarray(block, dtype=np.int32)
        if blk.ndim != 1:
            raise ValueError("block must be one id per SNP")
        if extra is None:
            ex, mem, ptr, E = None, capi.DMX_MEM_HOST, None, 0
        elif isinstance(extra, int):
            if n_extra is None:
                raise ValueError("a device `extra` needs n_extra")
            ex, mem, ptr, E = None, capi.DMX_MEM_DEVICE, extra, int(n_extra)
        else:
            ex = np.ascontiguousarray(extra, dtype=np.int32)
            if ex.ndim != 3 or ex.shape[0] != self.B or ex.shape[2] != 3:
                raise ValueError(f"extra must be [{self.B}][E][3]")
            mem, ptr, E = capi.DMX_MEM_HOST, (ex.ctypes.data if ex.size else None), ex.shape[1]
        rq = capi.BlockLlkRequest(self.B, blk.shape[0], int(n_blocks), E, blk.ctypes.data if blk.size else None, ptr, mem)
        check(self._L.dmx_engine_block_llk(self._h, C.byref(rq)))
        inf = self.block_llk_info()
        B, G = inf["n_cells"], inf["n_blocks"]
        col = np.zeros((B, G, inf["n_samples"])); l00 = np.zeros((B, G, inf["n_alpha"])); ext = np.zeros((B, G, inf["n_extra"]))
        n_snp = np.zeros((B, G), dtype=np.int32)
        check(self._L.dmx_engine_get_block_llk(self._h, col.ctypes.data, l00.ctypes.data, ext.ctypes.data, n_snp.ctypes.data))
        return dict(col=col, l00=l00, ext=ext, n_snp=n_snp)

    def block_llk_info(self) -> dict:
        """HIP-event time (ms) of the last block_llk's kernel, its result bytes, entry count and shape (dmx_engine_block_llk_info)."""
        r = capi.BlockLlkInfo()
        check(self._L.dmx_engine_block_llk_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.BlockLlkInfo._fields_ if n != "reserved"}

    def get_redrawn(self) -> dict:
        """The last redraw copied to the host (dmx_engine_get_redrawn): reads (uint8 [n_reads]) and geno (int8 [n_pairs][2]: the drawn
        genotypes of v1 and v2, -1 = not drawn)."""
        st = self.redrawn_pileup()
        reads = np.zeros(st.n_reads, dtype=np.uint8); geno = np.zeros((st.n_pairs, 2), dtype=np.int8)
        check(self._L.dmx_engine_get_redrawn(self._h, reads.ctypes.data if reads.size else None, geno.ctypes.data if geno.size else None))
        return {"reads": reads, "geno": geno}

    def _share_soup(self, rho, ambient):
        rh = amb = None
        if rho is not None:
            rh = np.ascontiguousarray(rho, dtype=np.float64)
            if rh.shape != (self.B,):
                raise ValueError(f"rho must be [{self.B}]")
        if ambient is not None:
            amb = np.ascontiguousarray(ambient, dtype=np.float64)
            if amb.ndim != 1:
                raise ValueError("ambient must be 1-D")
        return rh, amb, (len(amb) if amb is not None else self.S)

    def share_scan(self, anchors, rho=None, ambient=None, n_anchor=None):
        """dmx_engine_share_scan over the staged pileup: for anchors[b][t] (-1 = slot not used) and every other sample v, LL, LL' and LL'' in
        the share alpha of v's reads at alpha = 0, with a fraction rho[b] (None = 0) of the reads from a soup of ALT frequency ambient[i].
        `anchors` is a host array [B][T], or a device pointer (int) to B x n_anchor int32.  Returns (out[B][T][V][3] f64, n_snp[B][T] i32,
        n_read[B][T] i32)."""
        rh, amb, n_snps = self._share_soup(rho, ambient)
        if isinstance(anchors, int):
            if n_anchor is None:
                raise ValueError("device anchors need n_anchor=")
            an, mem, ptr, T = None, capi.DMX_MEM_DEVICE, anchors, int(n_anchor)
        else:
            an = np.ascontiguousarray(anchors, dtype=np.int32)
            if an.ndim != 2 or an.shape[0] != self.B:
                raise ValueError(f"anchors must be [{self.B}][T]")
            mem, ptr, T = capi.DMX_MEM_HOST, (an.ctypes.data if an.size else None), an.shape[1]
        rq = capi.ShareScanRequest(self.B, n_snps, T, mem, ptr, rh.ctypes.data if rh is not None and rh.size else None,
                                   amb.ctypes.data if amb is not None and amb.size else None)
        check(self._L.dmx_engine_share_scan(self._h, C.byref(rq)))
        out = np.zeros((self.B, T, self.V, 3))
        cnt = np.zeros((self.B, T, 2), dtype=np.int32)
        check(self._L.dmx_engine_get_share_scan(self._h, out.ctypes.data, cnt.ctypes.data))
        return out, cnt[:, :, 0].copy(), cnt[:, :, 1].copy()

    def share_fit(self, cand, rho=None, ambient=None, start: float = 0.5, tol: float = 1e-6, max_iter: int = 30, probe: float = -1.0,
                  n_cand=None) -> dict:
        """dmx_engine_share_fit over the staged pileup: for cand[b][c] = (v1, v2) (v1 = -1: slot not used) the share alpha_hat of v2's reads
        that maximises the doublet log-likelihood, by the safeguarded Newton iteration include/dmx.h states.  `cand` is a host array
        [B][C][2], or a device pointer (int) to B x n_cand x 2 int32.  Returns a dict of alpha, ll / d1 / d2 (at alpha_hat), ll0 / d10 / d20
        (at 0), ll1 / d11 / d21 (at 1), llp / d1p / d2p (at `probe`, when it is in [0, 1]) (f64 [B][C]) and n_eval, status, n_snp, n_read
        (i32 [B][C])."""
        rh, amb, n_snps = self._share_soup(rho, ambient)
        if isinstance(cand, int):
            if n_cand is None:
                raise ValueError("a device cand needs n_cand=")
            cd, mem, ptr, Cn = None, capi.DMX_MEM_DEVICE, cand, int(n_cand)
        else:
            cd = np.ascontiguousarray(cand, dtype=np.int32)
            if cd.ndim != 3 or cd.shape[0] != self.B or cd.shape[2] != 2:
                raise ValueError(f"cand must be [{self.B}][C][2]")
            mem, ptr, Cn = capi.DMX_MEM_HOST, (cd.ctypes.data if cd.size else None), cd.shape[1]
        rq = capi.ShareFitRequest(self.B, n_snps, Cn, mem, ptr, rh.ctypes.data if rh is not None and rh.size else None,
                                  amb.ctypes.data if amb is not None and amb.size else None, float(start), float(tol), float(probe), int(max_iter))
        check(self._L.dmx_engine_share_fit(self._h, C.byref(rq)))
        val = np.zeros((self.B, Cn, 13))
        cnt = np.zeros((self.B, Cn, 4), dtype=np.int32)
        check(self._L.dmx_engine_get_share_fit(self._h, val.ctypes.data, cnt.ctypes.data))
        names = ("alpha", "ll", "d1", "d2", "ll0", "d10", "d20", "ll1", "d11", "d21", "llp", "d1p", "d2p")
        out = {n: val[:, :, i].copy() for i, n in enumerate(names)}
        out.update({n: cnt[:, :, i].copy() for i, n in enumerate(("n_eval", "status", "n_snp", "n_read"))})
        return out

    def share_info(self) -> dict:
        """HIP-event times (ms) of the last share_scan / share_fit, their device bytes, entries and evaluations (dmx_engine_share_info)."""
        r = capi.ShareInfo()
        check(self._L.dmx_engine_share_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.ShareInfo._fields_ if n != "reserved"}

    def triplet_profile(self, base, shares, n_base=None):
        """dmx_engine_triplet over the staged pileup: LL[b][s][t][c] of barcode b as a triplet of the base pair base[b][s] = (v1, v2)
        (v1 = -1: slot not used) and the third donor c, with the read shares shares[t] = (w1, w2, w3) of v1, v2 and c.  `base` is a host
        array [B][C][2], or a device pointer (int) to B x n_base x 2 int32.
        Returns (ll[B][C][T][V] f64, n_snp[B][C][V] i32, n_read[B][C][V] i32)."""
        sh = np.ascontiguousarray(shares, dtype=np.float64)
        if sh.ndim != 2 or sh.shape[1] != 3:
            raise ValueError("shares must be [T][3]")
        if isinstance(base, int):
            if n_base is None:
                raise ValueError("a device base needs n_base=")
            bs, mem, ptr, Cn = None, capi.DMX_MEM_DEVICE, base, int(n_base)
        else:
            bs = np.ascontiguousarray(base, dtype=np.int32)
            if bs.ndim != 3 or bs.shape[0] != self.B or bs.shape[2] != 2:
                raise ValueError(f"base must be [{self.B}][C][2]")
            mem, ptr, Cn = capi.DMX_MEM_HOST, (bs.ctypes.data if bs.size else None), bs.shape[1]
        T = sh.shape[0]
        rq = capi.TripletRequest(self.B, mem, ptr, Cn, T, self.S, 0, sh.ctypes.data if sh.size else None)
        check(self._L.dmx_engine_triplet(self._h, C.byref(rq)))
        ll = np.zeros((self.B, Cn, T, self.V))
        n_snp = np.zeros((self.B, Cn, self.V), dtype=np.int32)
        n_read = np.zeros((self.B, Cn, self.V), dtype=np.int32)
        check(self._L.dmx_engine_get_triplet(self._h, ll.ctypes.data, n_snp.ctypes.data, n_read.ctypes.data))
        return ll, n_snp, n_read

    def triplet_info(self) -> dict:
        """HIP-event time (ms) of the last triplet profile and its size (dmx_engine_triplet_info)."""
        r = capi.TripletInfo()
        check(self._L.dmx_engine_triplet_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.TripletInfo._fields_ if not n.startswith("reserved")}

    def doublet_anchored(self, n_anchor: int = 2, anchors=None) -> None:
        """dmx_engine_doublet_anchored over the staged pileup: column 0 of the doublet grid, the n_anchor best singlets of every barcode
        as anchors (or the caller's `anchors`: a host array [B][T] with -1 = unused, or a device pointer (int) to B x n_anchor int32),
        every sample as the partner of every anchor in both orders, and K3's record over those entries.  STRICT arithmetic whatever
        the engine's mode; the full grid is never allocated.  Results: get_anchored()."""
        if anchors is None:
            an, mem, ptr, T = None, capi.DMX_MEM_HOST, None, int(n_anchor)
        elif isinstance(anchors, int):
            an, mem, ptr, T = None, capi.DMX_MEM_DEVICE, anchors, int(n_anchor)
        else:
            an = np.ascontiguousarray(anchors, dtype=np.int32)
            if an.ndim != 2 or an.shape[0] != self.B:
                raise ValueError(f"anchors must be [{self.B}][T]")
            mem, ptr, T = capi.DMX_MEM_HOST, (an.ctypes.data if an.size else None), an.shape[1]
            if ptr is None and self.B > 0:
                raise ValueError("anchors must have at least one column")
        rq = capi.AnchoredRequest(self.B, T, mem, 0, ptr)
        check(self._L.dmx_engine_doublet_anchored(self._h, C.byref(rq)))

    def get_anchored(self) -> dict:
        """The last anchored result (dmx_engine_get_anchored): anchors[B][T] i32, c0[B][V][A] = llksAB[j][0][n], pairs[B][T][V][2][A-1]
        with pairs[b][t][k][0][n-1] = llksAB[a_t][k][n] and pairs[b][t][k][1][n-1] = llksAB[k][a_t][n], llks00[B][A], summary[B]."""
        inf = self.anchored_info()
        B, V, A, T = inf["n_cells"], inf["n_samples"], inf["n_alpha"], inf["n_anchor"]
        anchors = np.zeros((B, T), dtype=np.int32)
        c0 = np.zeros((B, V, A))
        pairs = np.zeros((B, T, V, 2, A - 1))
        l00 = np.zeros((B, A))
        summ = np.zeros(B, dtype=capi.SUMMARY_DTYPE)
        check(self._L.dmx_engine_get_anchored(self._h, anchors.ctypes.data, c0.ctypes.data, pairs.ctypes.data, l00.ctypes.data, summ.ctypes.data))
        return dict(anchors=anchors, c0=c0, pairs=pairs, llks00=l00, summary=summ)

    def anchored_info(self) -> dict:
        """HIP-event times (ms) of the last anchored pass's kernels, its result bytes and entry count (dmx_engine_anchored_info)."""
        r = capi.AnchoredInfo()
        check(self._L.dmx_engine_anchored_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.AnchoredInfo._fields_ if not n.startswith("reserved")}

    def compose(self, parent, keep, seed: int, index_base: int = 0) -> dict:
        """dmx_engine_compose over the staged pileup: output barcode o takes the reads of cells parent[o][0] and parent[o][1] (-1 = none),
        each read kept iff its 32-bit hash is below keep[o][slot] (0 .. 2^32; 2^32 keeps all); output o is hashed as id index_base + o,
        so that a recipe composed in chunks gives the same barcodes.  Returns the info dict (compose_info)."""
        pr = np.ascontiguousarray(parent, dtype=np.int32)
        kp = np.ascontiguousarray(keep, dtype=np.uint64)
        if pr.ndim != 2 or pr.shape[1] != 2 or kp.shape != pr.shape:
            raise ValueError("parent and keep must both be [n_out][2]")
        rq = capi.ComposeRequest(pr.shape[0], 0, int(index_base), pr.ctypes.data if pr.size else None, kp.ctypes.data if kp.size else None,
                                 int(seed) & 0xFFFFFFFFFFFFFFFF)
        check(self._L.dmx_engine_compose(self._h, C.byref(rq)))
        return self.compose_info()

    def compose_info(self) -> dict:
        """Sizes, algorithmic bytes and HIP-event times (ms) of the last compose (dmx_engine_compose_info)."""
        r = capi.ComposeInfo()
        check(self._L.dmx_engine_compose_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.ComposeInfo._fields_ if n != "reserved"}

    def composed_pileup(self) -> capi.Pileup:
        """The composed pileup as a device-resident dmx_pileup (dmx_engine_composed_pileup) for another engine's set_pileup_struct or for
        demuxlet_run; the rd_* counters are NULL (a caller that needs them attaches host arrays).  Owned by this engine: valid until its
        next compose / set_pileup / close."""
        st = capi.Pileup()
        check(self._L.dmx_engine_composed_pileup(self._h, C.byref(st)))
        return st

    def composed_offsets(self):
        """(cell_pair_off, cell_read_off) of the composed pileup alone: N.SNP and the kept reads of every output barcode."""
        N = self.compose_info()["n_out"]
        po = np.zeros(N + 1, dtype=np.int64); ro = np.zeros(N + 1, dtype=np.int64)
        check(self._L.dmx_engine_get_composed(self._h, po.ctypes.data, ro.ctypes.data, None, None, None))
        return po, ro

    def get_composed(self) -> HostPileup:
        """The composed pileup copied to the host (dmx_engine_get_composed).  Its rd_totl = rd_pass = rd_uniq are SYNTHETIC: the kept reads
        of each barcode — a composed barcode has no scan behind it, so there is no count of reads that failed a filter or repeated a UMI."""
        inf = self.compose_info()
        N, P, R = inf["n_out"], inf["n_pairs"], inf["n_reads"]
        po = np.zeros(N + 1, dtype=np.int64); ro = np.zeros(N + 1, dtype=np.int64)
        snp = np.zeros(P, dtype=np.int32)
        nrd = np.zeros(P, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32}[inf["nrd_width"]])
        reads = np.zeros(R, dtype=np.uint8)
        check(self._L.dmx_engine_get_composed(self._h, po.ctypes.data, ro.ctypes.data, snp.ctypes.data if P else None,
                                              nrd.ctypes.data if P else None, reads.ctypes.data if R else None))
        kept = np.diff(ro).astype(np.int32)
        return HostPileup(N, self.S, po, ro, snp, nrd, reads, kept, kept.copy(), kept.copy())

    def _census_group(self, group, n_groups):
        """(keep-alive array, memory, pointer, G) of a census `group`: a host array [B] or a device pointer (int) to B int32."""
        if isinstance(group, int):
            if n_groups is None:
                raise ValueError("a device group needs n_groups=")
            return None, capi.DMX_MEM_DEVICE, group, int(n_groups)
        gr = np.ascontiguousarray(group, dtype=np.int32)
        if gr.shape != (self.B,):
            raise ValueError(f"group must be [{self.B}]")
        G = int(n_groups) if n_groups is not None else (int(gr.max()) + 1 if gr.size and gr.max() >= 0 else 1)
        return gr, capi.DMX_MEM_HOST, (gr.ctypes.data if gr.size else None), G

    def census_step(self, group, w, n_groups=None):
        """dmx_engine_census_step over the staged pileup: one pass of the mixture-proportion EM at the shares w[G][V] for the groups
        group[b] in [-1, G) (-1 = barcode not used; a host array, or a device pointer (int) to B int32 with n_groups=).
        Returns (acc[G][V] f64, ll[G] f64, gap[G] f64, n_read[G] i64, n_pair[G] i64); the EM image of w is w * acc / n_read."""
        gr, mem, ptr, G = self._census_group(group, n_groups)
        ww = np.ascontiguousarray(w, dtype=np.float64)
        if ww.ndim == 1:
            ww = ww[None, :]
        if ww.shape != (G, self.V):
            raise ValueError(f"w must be [{G}][{self.V}]")
        acc = np.zeros((G, self.V)); ll = np.zeros(G); gap = np.zeros(G)
        n_read = np.zeros(G, dtype=np.int64); n_pair = np.zeros(G, dtype=np.int64)
        rq = capi.CensusStepRequest(self.B, mem, ptr, G, self.V, ww.ctypes.data, acc.ctypes.data, ll.ctypes.data, gap.ctypes.data,
                                    n_read.ctypes.data, n_pair.ctypes.data)
        check(self._L.dmx_engine_census_step(self._h, C.byref(rq)))
        return acc, ll, gap, n_read, n_pair

    def census(self, group, n_groups=None, w0=None, tol: float = 1e-4, max_steps: int = 2000, accelerate: bool = True,
               gap_on_support: bool = False) -> dict:
        """dmx_engine_census over the staged pileup: the maximum-likelihood donor shares of every group, by SQUAREM (or plain EM with
        accelerate=False) from w0[G][V] (None = uniform), each group stopping at duality gap <= tol or after max_steps passes.
        gap_on_support=True takes the gap's maximum over the donors with w0 > 0 only (the duality gap of the problem constrained to the
        start's support: the stopping rule of a refit with donors held at 0).
        Returns a dict: w[G][V], ll[G], gap[G], n_steps[G], converged[G], n_read[G], n_pair[G]."""
        gr, mem, ptr, G = self._census_group(group, n_groups)
        start = None
        if w0 is not None:
            start = np.ascontiguousarray(w0, dtype=np.float64)
            if start.ndim == 1:
                start = start[None, :]
            if start.shape != (G, self.V):
                raise ValueError(f"w0 must be [{G}][{self.V}]")
        rq = capi.CensusRequest(self.B, mem, ptr, G, self.V, start.ctypes.data if start is not None else None, float(tol), int(max_steps),
                                1 if accelerate else 0)
        if gap_on_support:
            rq.reserved[0] = 1
        check(self._L.dmx_engine_census(self._h, C.byref(rq)))
        w = np.zeros((G, self.V)); ll = np.zeros(G); gap = np.zeros(G)
        n_steps = np.zeros(G, dtype=np.int32); conv = np.zeros(G, dtype=np.int32)
        n_read = np.zeros(G, dtype=np.int64); n_pair = np.zeros(G, dtype=np.int64)
        check(self._L.dmx_engine_get_census(self._h, w.ctypes.data, ll.ctypes.data, gap.ctypes.data, n_steps.ctypes.data, conv.ctypes.data,
                                            n_read.ctypes.data, n_pair.ctypes.data))
        return dict(w=w, ll=ll, gap=gap, n_steps=n_steps, converged=conv, n_read=n_read, n_pair=n_pair)

    def census_info(self) -> dict:
        """HIP-event times (ms) of the last census pass and dosage kernel, passes run, table sizes and invalid SNPs (dmx_engine_census_info)."""
        r = capi.CensusInfo()
        check(self._L.dmx_engine_census_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.CensusInfo._fields_ if n != "reserved"}

    def census_fisher(self, group, w, n_groups=None) -> dict:
        """dmx_engine_census_fisher over the staged pileup: the observed information of the shares at w[G][V] and the per-barcode
        scores (include/dmx.h), V <= 128.  `group` as for census_step.  Returns a dict: H[G][V][V] (symmetric),
        score[B][V] and n_read_b[B] (zero for barcodes of group -1), acc[G][V], ll[G], n_read[G], n_pair[G] (census_step's bits)."""
        gr, mem, ptr, G = self._census_group(group, n_groups)
        ww = np.ascontiguousarray(w, dtype=np.float64)
        if ww.ndim == 1:
            ww = ww[None, :]
        if ww.shape != (G, self.V):
            raise ValueError(f"w must be [{G}][{self.V}]")
        H = np.zeros((G, self.V, self.V)); score = np.zeros((self.B, self.V)); n_b = np.zeros(self.B, dtype=np.int64)
        acc = np.zeros((G, self.V)); ll = np.zeros(G)
        n_read = np.zeros(G, dtype=np.int64); n_pair = np.zeros(G, dtype=np.int64)
        rq = capi.CensusFisherRequest(self.B, mem, ptr, G, self.V, ww.ctypes.data, H.ctypes.data, score.ctypes.data if score.size else None,
                                      n_b.ctypes.data if n_b.size else None, acc.ctypes.data, ll.ctypes.data, n_read.ctypes.data,
                                      n_pair.ctypes.data)
        check(self._L.dmx_engine_census_fisher(self._h, C.byref(rq)))
        return dict(H=H, score=score, n_read_b=n_b, acc=acc, ll=ll, n_read=n_read, n_pair=n_pair)

    def census_fisher_info(self) -> dict:
        """HIP-event time (ms) of the last census_fisher call's kernels, partial bytes, chunks, entry blocks and entries."""
        r = capi.CensusFisherInfo()
        check(self._L.dmx_engine_census_fisher_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.CensusFisherInfo._fields_ if n != "reserved"}

    def _prior_request(self, grid, mask, n_cells=None):
        """(request, keep-alive list) of a prior call.  grid: None = the engine's llksAB of the last run_doublet; a host array
        [B][V][V][A]; or a device pointer (int) to one, with n_cells=.  mask: None, or [B] (0 = leave the barcode out)."""
        keep = []
        if grid is None:
            B, mem, ptr = self.B, capi.DMX_MEM_HOST, None
        elif isinstance(grid, int):
            if n_cells is None:
                raise ValueError("a device grid needs n_cells=")
            B, mem, ptr = int(n_cells), capi.DMX_MEM_DEVICE, grid
        else:
            gr = np.ascontiguousarray(grid, dtype=np.float64)
            if gr.ndim != 4 or gr.shape[1:] != (self.V, self.V, self.A):
                raise ValueError(f"grid must be [B][{self.V}][{self.V}][{self.A}]")
            keep.append(gr)
            B, mem, ptr = gr.shape[0], capi.DMX_MEM_HOST, (gr.ctypes.data if gr.size else None)
            if ptr is None:
                raise ValueError("grid has no barcode")
        mp = None
        if mask is not None:
            mk = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            if mk.shape != (B,):
                raise ValueError(f"mask must be [{B}]")
            keep.append(mk)
            mp = mk.ctypes.data if mk.size else None
        rq = capi.PriorRequest(B, self.V, self.A, mem, ptr, mp)
        return rq, keep

    def prior_step(self, pi, d: float, grid=None, mask=None, n_cells=None, rows: bool = False) -> dict:
        """dmx_engine_prior_step: one E + M of the empirical-Bayes prior fit at shares pi[V] (any positive scale) and doublet rate d
        (include/dmx.h).  `grid`, `mask`, `n_cells` as in _prior_request.  Returns a dict: N[V], hom, het, ll,
        b_in, pi_next[V], d_next, and with rows=True rows[B][V + 3] (N contributions | hom | het | log E_b) and flags[B]."""
        rq, keep = self._prior_request(grid, mask, n_cells)
        p = np.ascontiguousarray(pi, dtype=np.float64)
        if p.shape != (self.V,):
            raise ValueError(f"pi must be [{self.V}]")
        check(self._L.dmx_engine_prior_step(self._h, C.byref(rq), p.ctypes.data, float(d)))
        self._prior_step_B = rq.n_cells             # (a refused call leaves the last step's results, and its count, as they were)
        return self.get_prior_step(rows=rows)

    def get_prior_step(self, rows: bool = True) -> dict:
        """The last prior_step's results (dmx_engine_get_prior_step).  They stay readable after a prior_call and after a call that was
        refused for its arguments, the engine's state or its memory need; a prior_fit overwrites the rows, so they are gone after one."""
        self.prior_info()                            # (DMX_ERR_STATE before any prior call)
        B = getattr(self, "_prior_step_B", 0)       # the last step's barcodes: a later prior_call may have had another count
        N = np.zeros(self.V); pn = np.zeros(self.V)
        hom = C.c_double(); het = C.c_double(); ll = C.c_double(); dn = C.c_double(); b_in = C.c_int32()
        rw = np.zeros((B, self.V + 3)) if rows else None
        fl = np.zeros(B, dtype=np.uint8) if rows else None
        check(self._L.dmx_engine_get_prior_step(self._h, N.ctypes.data, C.byref(hom), C.byref(het), C.byref(ll), C.byref(b_in), pn.ctypes.data,
                                                C.byref(dn), rw.ctypes.data if rows else None, fl.ctypes.data if rows else None))
        r = dict(N=N, hom=hom.value, het=het.value, ll=ll.value, b_in=b_in.value, pi_next=pn, d_next=dn.value)
        if rows:
            r.update(rows=rw, flags=fl)
        return r

    def prior_fit(self, grid=None, mask=None, n_cells=None, pi0=None, d0: float = 0.1, max_iter: int = 200, tol: float = 1e-6,
                  fix_pi: bool = False, fix_d: bool = False) -> dict:
        """dmx_engine_prior_fit: the EM loop inside the library from (pi0 (None = uniform), d0); it stops after the iteration whose
        log-likelihood gain is below tol x B_in (tol <= 0: never) or after max_iter, then evaluates once more at the final (pi, d).
        Returns a dict: pi[V], d, ll, N[V], hom, het (at the final pi, d), b_in, n_iter, converged, ll_trace[n_iter], d_trace[n_iter]
        (iteration t's log-likelihood and the rate it was evaluated at)."""
        rq, keep = self._prior_request(grid, mask, n_cells)
        if pi0 is not None:
            p0 = np.ascontiguousarray(pi0, dtype=np.float64)
            if p0.shape != (self.V,):
                raise ValueError(f"pi0 must be [{self.V}]")
            keep.append(p0)
            rq.pi0 = p0.ctypes.data
        rq.d0, rq.tol, rq.max_iter, rq.fix_pi, rq.fix_d = float(d0), float(tol), int(max_iter), int(bool(fix_pi)), int(bool(fix_d))
        check(self._L.dmx_engine_prior_fit(self._h, C.byref(rq)))
        pi = np.zeros(self.V); N = np.zeros(self.V)
        d = C.c_double(); ll = C.c_double(); hom = C.c_double(); het = C.c_double()
        n_iter = C.c_int32(); conv = C.c_int32(); b_in = C.c_int32()
        llt = np.zeros(int(max_iter)); dt = np.zeros(int(max_iter))
        check(self._L.dmx_engine_get_prior_fit(self._h, pi.ctypes.data, C.byref(d), C.byref(ll), C.byref(n_iter), C.byref(conv), C.byref(b_in),
                                               N.ctypes.data, C.byref(hom), C.byref(het), llt.ctypes.data, dt.ctypes.data, int(max_iter)))
        n = n_iter.value
        return dict(pi=pi, d=d.value, ll=ll.value, N=N, hom=hom.value, het=het.value, b_in=b_in.value, n_iter=n, converged=bool(conv.value),
                    ll_trace=llt[:n].copy(), d_trace=dt[:n].copy())

    def prior_call(self, pi, d: float, grid=None, mask=None, n_cells=None) -> np.ndarray:
        """dmx_engine_prior_call + dmx_engine_get_prior_calls: the per-barcode records at (pi, d), a structured array [B] of
        capi.PRIOR_CALL_DTYPE (log_e, p_sng, p_het, p_hom, p_sng1, p_sng2, p_dbl1, i_sng1, i_sng2, j_dbl, k_dbl, n_dbl, flag)."""
        rq, keep = self._prior_request(grid, mask, n_cells)
        p = np.ascontiguousarray(pi, dtype=np.float64)
        if p.shape != (self.V,):
            raise ValueError(f"pi must be [{self.V}]")
        check(self._L.dmx_engine_prior_call(self._h, C.byref(rq), p.ctypes.data, float(d)))
        out = np.zeros(rq.n_cells, dtype=capi.PRIOR_CALL_DTYPE)
        check(self._L.dmx_engine_get_prior_calls(self._h, out.ctypes.data))
        return out

    def prior_info(self) -> dict:
        """HIP-event times (ms) of the last prior kernels, the last fit's iterations and summed time, and the grid bytes one iteration
        reads (dmx_engine_prior_info)."""
        r = capi.PriorInfo()
        check(self._L.dmx_engine_prior_info(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in capi.PriorInfo._fields_ if n != "reserved"}

    def device_view(self) -> capi.DeviceView:
        v = capi.DeviceView()
        check(self._L.dmx_engine_device_view(self._h, C.byref(v)))
        return v

    def kernel_times(self) -> capi.KernelTimes:
        t = capi.KernelTimes()
        check(self._L.dmx_engine_last_kernel_times(self._h, C.byref(t)))
        return t

    def mean_kernel_times(self, reset: bool = False) -> capi.KernelTimeMeans:
        """Mean HIP-event time of K1, K2, K3 and K3b over the launches since the last reset (at most the last 16)."""
        t = capi.KernelTimeMeans()
        check(self._L.dmx_engine_mean_kernel_times(self._h, int(reset), C.byref(t)))
        return t

    def reset_kernel_times(self) -> None:
        check(self._L.dmx_engine_mean_kernel_times(self._h, 1, None))

    def kernel_names(self) -> dict:
        """Which kernels the last run launched (dmx_engine_kernel_names): {'singlet', 'doublet', 'certify': rocprofv3-style names, 'k1_placement'}."""
        n = capi.KernelNames()
        check(self._L.dmx_engine_kernel_names(self._h, C.byref(n)))
        return {"singlet": n.singlet.decode(), "doublet": n.doublet.decode(), "certify": n.certify.decode(), "k1_placement": int(n.k1_placement)}

    def algorithmic_bytes(self) -> capi.KernelBytes:
        b = capi.KernelBytes()
        check(self._L.dmx_engine_algorithmic_bytes(self._h, C.byref(b)))
        return b


class Inflater:
    """BGZF members inflated on one MI355X (dmx_inflater_*): raw DEFLATE streams in, bytes and one status per
    member out.  status 0 = accepted with zlib's bytes; anything else = refused, to be inflated by the caller (no checksum is computed)."""

    PAD = 64          # bytes between two members' slots in the buffers this class packs (guards; the contract needs 8 zero bytes after an input)

    def __init__(self, device: int = 0, max_members: int = 1024, max_in_bytes: int = 1 << 26, max_out_bytes: int = 1 << 26):
        self._L = capi.load()
        h = C.c_void_p()
        check(self._L.dmx_inflater_create(device, max_members, max_in_bytes, max_out_bytes, C.byref(h)))
        self._h = h
        self._keep = {}

    def close(self):
        if getattr(self, "_h", None):
            self._L.dmx_inflater_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @staticmethod
    def pack(streams: Sequence[bytes]):
        """The members' deflate data in one buffer: each at a multiple of 16, followed by at least PAD zero bytes.  -> (buf u8, off i64, len i32)"""
        ln = np.array([len(z) for z in streams], dtype=np.int32)
        slot = (ln.astype(np.int64) + Inflater.PAD + 15) // 16 * 16
        off = np.concatenate([[0], np.cumsum(slot)[:-1]]).astype(np.int64) if len(streams) else np.zeros(0, np.int64)
        buf = np.zeros(int(slot.sum()) + 16, dtype=np.uint8)
        for z, o in zip(streams, off):
            buf[o:o + len(z)] = np.frombuffer(z, dtype=np.uint8)
        return buf, off, ln

    def submit(self, slot: int, buf: np.ndarray, in_off, in_len, out: np.ndarray, out_off, out_len) -> None:
        """dmx_inflater_submit; the arrays are kept alive until wait(slot)."""
        a = [np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(in_off, np.int64), np.ascontiguousarray(in_len, np.int32),
             out, np.ascontiguousarray(out_off, np.int64), np.ascontiguousarray(out_len, np.int32)]
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
        n = len(a[2])
        assert len(a[1]) == n and len(a[4]) == n and len(a[5]) == n
        check(self._L.dmx_inflater_submit(self._h, slot, n, *(x.ctypes.data for x in a)))
        self._keep[slot] = (a, n)

    def wait(self, slot: int):
        """dmx_inflater_wait -> (status i32 [n], info dict)"""
        a, n = self._keep.get(slot, (None, 0))
        status = np.full(max(n, 1), -1, dtype=np.int32)
        info = capi.InflaterInfo()
        check(self._L.dmx_inflater_wait(self._h, slot, status.ctypes.data, C.byref(info)))
        self._keep.pop(slot, None)
        return status[:n], {k: getattr(info, k) for k, _ in capi.InflaterInfo._fields_ if k != "reserved"}

    def run(self, streams: Sequence[bytes], out_lens: Sequence[int], guard: int = 0, fill: int = 0):
        """Every stream i inflated into out_lens[i] bytes -> (list of bytes, status, info, out buffer, out offsets).  With guard > 0 the
        output slots are separated (and preceded and followed) by `guard` bytes of `fill`, for the caller to look at afterwards."""
        buf, off, ln = self.pack(streams)
        ol = np.asarray(out_lens, dtype=np.int32)
        ooff = (guard + np.concatenate([[0], np.cumsum(ol.astype(np.int64) + guard)[:-1]])).astype(np.int64) if len(ol) else np.zeros(0, np.int64)
        out = np.full(int(ol.astype(np.int64).sum()) + guard * (len(ol) + 1) + 1, fill, dtype=np.uint8)
        self.submit(0, buf, off, ln, out, ooff, ol)
        status, info = self.wait(0)
        return [out[o:o + n].tobytes() for o, n in zip(ooff, ol)], status, info, out, ooff


def _cstrs(strs: Sequence[str]):
    keep = [s.encode() for s in strs]
    arr = (C.c_char_p * max(1, len(keep)))(*keep) if keep else (C.c_char_p * 1)()
    return arr, keep


@dataclass
class FinalArgs:
    barcodes: Sequence[str]
    sample_ids: Sequence[str]
    alphas: Sequence[float]
    doublet_prior: float
    rd_totl: np.ndarray
    rd_pass: np.ndarray
    rd_uniq: np.ndarray
    n_snp: np.ndarray
    min_total: int = 0
    min_uniq: int = 0
    min_snp: int = 0
    write_pair: bool = False


def _final_struct(fa: FinalArgs, llks=None, llk0s=None, grid=None, l00=None, tie_pileup: Optional[HostPileup] = None,
                  tie_g: Optional[np.ndarray] = None, cell_grids=None):
    keep = []
    alphas = np.ascontiguousarray(fa.alphas, dtype=np.float64)
    bc, k1 = _cstrs(fa.barcodes)
    sm, k2 = _cstrs(fa.sample_ids)
    arrs = [np.ascontiguousarray(x, dtype=np.int32) for x in (fa.rd_totl, fa.rd_pass, fa.rd_uniq, fa.n_snp)]
    keep += [alphas, bc, k1, sm, k2, arrs]

    def p(x):
        if x is None:
            return None
        x = np.ascontiguousarray(x, dtype=np.float64)
        keep.append(x)
        return x.ctypes.data

    tp = None
    if tie_pileup is not None:
        st = tie_pileup.as_struct()
        keep += [st, tie_pileup]
        tp = C.addressof(st)
        tie_g = np.ascontiguousarray(tie_g, dtype=np.float32)
        keep.append(tie_g)
    fin = capi.FinalInput(len(fa.barcodes), len(fa.sample_ids), len(alphas), alphas.ctypes.data, fa.doublet_prior,
                          fa.min_total, fa.min_uniq, fa.min_snp, int(fa.write_pair), C.cast(bc, C.c_void_p),
                          C.cast(sm, C.c_void_p), arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data,
                          arrs[3].ctypes.data, p(llks), p(llk0s), p(grid), p(l00), tp,
                          tie_g.ctypes.data if tie_pileup is not None else None, 0.0)
    fin._cell_grid = None
    if cell_grids:                                   # {cell id: llksAB[V][V][A]} of the near-tie-flagged barcodes
        ptrs = (C.c_void_p * len(fa.barcodes))()     # (an argument of dmx_write_doublet_summary_grids since ABI 7, not a member of the struct)
        for c, gr in cell_grids.items():
            gr = np.ascontiguousarray(gr, dtype=np.float64)
            assert gr.size == len(fa.sample_ids) ** 2 * len(alphas)
            keep.append(gr)
            ptrs[int(c)] = gr.ctypes.data
        keep.append(ptrs)
        fin._cell_grid = C.cast(ptrs, C.c_void_p)
    return fin, keep


def write_single(fa: FinalArgs, llks, llk0s, path: str) -> None:
    fin, keep = _final_struct(fa, llks=llks, llk0s=llk0s)
    check(capi.load().dmx_write_single(C.byref(fin), path.encode()))


def write_doublet(fa: FinalArgs, grid, l00, out_prefix: str, tie_pileup: Optional[HostPileup] = None,
                  tie_g: Optional[np.ndarray] = None) -> None:
    fin, keep = _final_struct(fa, grid=grid, l00=l00, tie_pileup=tie_pileup, tie_g=tie_g)
    check(capi.load().dmx_write_doublet(C.byref(fin), out_prefix.encode()))


def near_tie_cells(summary: np.ndarray) -> np.ndarray:
    """ids of the covered cells whose K3 record carries DMX_CELL_NEAR_DOUBLET / _NEAR_SINGLET: a decision of theirs sits within 1e-7 of
    an alternative other than the alpha = 0.5 mirror, and the writers decide it from the cell's grid (Engine.get_cell_grids)."""
    return np.flatnonzero(((summary["flags"] & (capi.DMX_CELL_NEAR_DOUBLET | capi.DMX_CELL_NEAR_SINGLET)) != 0) & (summary["n_pairs"] > 0)).astype(np.int32)


def write_doublet_summary(fa: FinalArgs, sing, l00, summary, out_prefix: str, tie_pileup: Optional[HostPileup] = None,
                          tie_g: Optional[np.ndarray] = None, cell_grids=None) -> None:
    """.sing2/.best from the per-cell records (K3 summaries) instead of the grid — what a multi-GPU run gathers.  `cell_grids`
    {cell id: llksAB[V][V][A]} carries the grids of the near-tie-flagged barcodes (near_tie_cells); without them and with the tie
    pileup such a barcode's grid is re-evaluated on the host."""
    fin, keep = _final_struct(fa, l00=l00, tie_pileup=tie_pileup, tie_g=tie_g, cell_grids=cell_grids)
    sing = np.ascontiguousarray(sing, dtype=np.float64)
    summary = np.ascontiguousarray(summary, dtype=capi.SUMMARY_DTYPE)
    if fin._cell_grid is not None:
        check(capi.load().dmx_write_doublet_summary_grids(C.byref(fin), sing.ctypes.data, summary.ctypes.data, fin._cell_grid, out_prefix.encode()))
    else:
        check(capi.load().dmx_write_doublet_summary(C.byref(fin), sing.ctypes.data, summary.ctypes.data, out_prefix.encode()))


def resolve_tie_order(summary: np.ndarray) -> int:
    """dmx_resolve_tie_order: DMX_CELL_ORDER_RESOLVABLE records -> certified ones, in place (the host libm's log() decides).
    Returns how many stayed unresolved."""
    assert summary.dtype == capi.SUMMARY_DTYPE and summary.flags["C_CONTIGUOUS"]
    return check(capi.load().dmx_resolve_tie_order(summary.ctypes.data, len(summary)))


def demuxlet_run(store, g: np.ndarray, sample_ids: Sequence[str], alphas: Sequence[float], out_prefix: str,
                 doublet_prior: float = 0.5, min_total: int = 0, min_uniq: int = 0, min_snp: int = 0,
                 write_pair: bool = False, device: int = 0, arbiter: bool = True, n_gpus: int = 1, mode: int = capi.DMX_MODE_STRICT,
                 barcodes: Optional[Sequence[str]] = None, timing: bool = False):
    """cmd_cram_demuxlet.cpp:390-881 in one call (dmx_demuxlet_run).  `store` is a Store, or a frozen pileup — a HostPileup or a
    capi.Pileup struct (device-resident arrays: memory = DMX_MEM_DEVICE, one GPU) — together with `barcodes` (dmx_job.pileup).
    With timing=True returns the stage seconds (dmx_job_timing) as a dict."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    al = np.ascontiguousarray(alphas, dtype=np.float64)
    sm, keep = _cstrs(sample_ids)
    tm = capi.JobTiming()
    if isinstance(store, (HostPileup, capi.Pileup)):
        # a frozen pileup: host arrays (HostPileup) or a dmx_pileup struct as it is — DMX_MEM_DEVICE: the five arrays in HBM, the
        # rd_* counters host memory (the caller keeps whatever the pointers refer to alive)
        st = store.as_struct() if isinstance(store, HostPileup) else store
        bc, keep_b = _cstrs(barcodes)
        job = capi.Job(None, g.ctypes.data, g.shape[1], C.cast(sm, C.c_void_p), len(al), al.ctypes.data, doublet_prior,
                       min_total, min_uniq, min_snp, int(write_pair), out_prefix.encode(), device, int(arbiter), n_gpus, mode,
                       C.addressof(st), C.cast(bc, C.c_void_p), C.addressof(tm) if timing else None)
    else:
        job = capi.Job(store.handle, g.ctypes.data, g.shape[1], C.cast(sm, C.c_void_p), len(al), al.ctypes.data, doublet_prior,
                       min_total, min_uniq, min_snp, int(write_pair), out_prefix.encode(), device, int(arbiter), n_gpus, mode,
                       None, None, C.addressof(tm) if timing else None)
    check(capi.load().dmx_demuxlet_run(C.byref(job)))
    if timing:
        return {name: getattr(tm, name) for name, _ in capi.JobTiming._fields_}
