"""ctypes binding of libdmx.so — a 1:1 mirror of include/dmx.h (no logic here beyond marshalling).

The library is loaded lazily from demuxlet_amd/libdmx.so (built in-tree by demuxlet_amd/build.py).  There is no Python
or CPU fallback for the engine: if the library or the GPU is missing, calls raise DmxError."""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Optional

import numpy as np

import os

LIB_PATH = Path(os.environ.get("DMX_LIB", Path(__file__).resolve().parent / "libdmx.so"))   # DMX_LIB: kernel experiments only

DMX_OK = 0
DMX_ERR_ARG, DMX_ERR_HIP, DMX_ERR_STATE, DMX_ERR_IO, DMX_ERR_NOGPU, DMX_ERR_NOMEM = -1, -2, -3, -4, -5, -6   # dmx_status (include/dmx.h)
DMX_MEM_HOST, DMX_MEM_DEVICE = 0, 1
DMX_MODE_STRICT = 0
DMX_MODE_FAST = 1
DMX_CELL_NEAR_DOUBLET, DMX_CELL_NEAR_SINGLET, DMX_CELL_ORDER_CERTIFIED, DMX_CELL_ORDER_RESOLVABLE, DMX_CELL_NEAR_RULE = 1, 2, 4, 8, 16
DMX_ENGINE_NO_CERTIFY = 1

# every symbol include/dmx.h declares (tests/test_abi.py checks the header against this list and the .so against both)
SYMBOLS = [
    "dmx_abi_version", "dmx_last_error", "dmx_device_warm_up", "dmx_phred_tables", "dmx_geno_from_gt", "dmx_geno_from_pl", "dmx_geno_from_gp",
    "dmx_store_new", "dmx_store_free", "dmx_store_add_snp", "dmx_store_add_cell", "dmx_store_count_read",
    "dmx_store_add_read", "dmx_store_n_cells", "dmx_store_n_snps", "dmx_store_barcode", "dmx_store_freeze",
    "dmx_engine_create", "dmx_engine_destroy", "dmx_engine_set_stream", "dmx_engine_set_phred_tables",
    "dmx_engine_set_genotypes", "dmx_engine_set_pileup", "dmx_engine_run_singlet", "dmx_engine_run_doublet", "dmx_engine_run",
    "dmx_engine_sync", "dmx_engine_get_singlet", "dmx_engine_get_doublet", "dmx_engine_device_view",
    "dmx_engine_last_kernel_times", "dmx_engine_algorithmic_bytes", "dmx_write_single", "dmx_write_doublet",
    "dmx_demuxlet_run", "dmx_debug_device_log", "dmx_debug_device_log2", "dmx_debug_device_div", "dmx_debug_log_rate", "dmx_engine_get_sing", "dmx_engine_get_cell_grids", "dmx_write_doublet_summary", "dmx_debug_log_dd",
    "dmx_resolve_tie_order", "dmx_engine_mean_kernel_times", "dmx_store_add_batch", "dmx_write_doublet_summary_grids", "dmx_engine_kernel_names", "dmx_debug_device_log2_lite", "dmx_debug_device_log2_lite32", "dmx_debug_device_log2_mirror",
    "dmx_engine_format_pair", "dmx_pair_text_get_info", "dmx_pair_text_get_scalars", "dmx_pair_text_read", "dmx_pair_text_free",
    "dmx_engine_refine_genotypes", "dmx_engine_get_refined", "dmx_engine_refined_device_ptr", "dmx_engine_refine_info",
    "dmx_engine_cluster_stage", "dmx_engine_cluster_mstep", "dmx_engine_cluster_estep", "dmx_engine_get_cluster", "dmx_engine_get_cluster_stage",
    "dmx_engine_cluster_device_ptr", "dmx_engine_cluster_info",
    "dmx_engine_cluster_doublet", "dmx_engine_get_cluster_doublet", "dmx_engine_cluster_estep_doublet", "dmx_engine_cluster_doublet_info",
    "dmx_engine_cluster_merge_score", "dmx_engine_cluster_estep_grouped", "dmx_engine_cluster_sm_info",
    "dmx_engine_cluster_evidence", "dmx_engine_cluster_hard", "dmx_engine_get_cluster_hard", "dmx_engine_cluster_hard_device_ptr", "dmx_engine_cluster_merge_columns",
    "dmx_engine_cluster_k_info",
    "dmx_engine_cluster_set_known", "dmx_engine_cluster_estep_known", "dmx_engine_cluster_mstep_window", "dmx_engine_get_cluster_known",
    "dmx_engine_cluster_known_info",
    "dmx_engine_ambient", "dmx_engine_get_ambient", "dmx_engine_ambient_info",
    "dmx_engine_ambient_doublet", "dmx_engine_get_ambient_doublet", "dmx_engine_ambient_doublet_info",
    "dmx_engine_triplet", "dmx_engine_get_triplet", "dmx_engine_triplet_info",
    "dmx_engine_compose", "dmx_engine_composed_pileup", "dmx_engine_get_composed", "dmx_engine_compose_info",
    "dmx_engine_census_step", "dmx_engine_census", "dmx_engine_get_census", "dmx_engine_census_info",
    "dmx_engine_census_fisher", "dmx_engine_census_fisher_info",
    "dmx_engine_doublet_anchored", "dmx_engine_get_anchored", "dmx_engine_anchored_info",
    "dmx_engine_prior_step", "dmx_engine_get_prior_step", "dmx_engine_prior_fit", "dmx_engine_get_prior_fit",
    "dmx_engine_prior_call", "dmx_engine_get_prior_calls", "dmx_engine_prior_info",
    "dmx_engine_fit", "dmx_engine_get_fit", "dmx_engine_fit_info",
    "dmx_engine_share_scan", "dmx_engine_get_share_scan", "dmx_engine_share_fit", "dmx_engine_get_share_fit", "dmx_engine_share_info",
    "dmx_engine_site_fit", "dmx_engine_get_site_fit", "dmx_engine_site_fit_info",
    "dmx_engine_redraw", "dmx_engine_redrawn_pileup", "dmx_engine_get_redrawn", "dmx_engine_redraw_info",
    "dmx_engine_geno_compare", "dmx_engine_get_geno_compare", "dmx_engine_geno_compare_info",
    "dmx_engine_block_llk", "dmx_engine_get_block_llk", "dmx_engine_block_llk_info",
    "dmx_inflater_create", "dmx_inflater_free", "dmx_inflater_submit", "dmx_inflater_wait", "dmx_inflater_run",
    "dmx_inflater_pin", "dmx_inflater_unpin",
]
DMX_PRIOR_MASKED, DMX_PRIOR_BAD = 1, 2


class PairOverride(C.Structure):      # dmx_pair_override
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("n", C.c_int32), ("reserved", C.c_int32), ("llk_ab", C.c_double), ("llk_ba", C.c_double)]


class PairPatch(C.Structure):         # dmx_pair_patch
    _fields_ = [("offset", C.c_int64), ("value", C.c_double), ("out_cell", C.c_int32), ("singlet", C.c_int32)]


class PairScalars(C.Structure):       # dmx_pair_scalars
    _fields_ = [("max_llk", C.c_double), ("sum_single", C.c_double), ("sum_double", C.c_double)]


class PairRequest(C.Structure):       # dmx_pair_request
    _fields_ = [("n_out", C.c_int32), ("cells", C.c_void_p), ("barcodes", C.c_void_p), ("sample_ids", C.c_void_p), ("host_rows", C.c_void_p), ("ovr", C.c_void_p)]


class PairTextInfo(C.Structure):      # dmx_pair_text_info
    _fields_ = [("n_bytes", C.c_int64), ("n_out", C.c_int32), ("n_patches", C.c_int32), ("cell_off", C.POINTER(C.c_int64)), ("cell_flag", C.POINTER(C.c_uint8)),
                ("patches", C.POINTER(PairPatch)), ("format_ms", C.c_double)]


class RefineRequest(C.Structure):     # dmx_refine_request
    _fields_ = [("n_cells", C.c_int32), ("assign_memory", C.c_int32), ("assign", C.c_void_p), ("n_snps", C.c_int32), ("reserved0", C.c_int32),
                ("prior", C.c_void_p), ("floor", C.c_double), ("reserved", C.c_int32 * 4)]


class RefineInfo(C.Structure):        # dmx_refine_info
    _fields_ = [("blocks_ms", C.c_double), ("partial_ms", C.c_double), ("finish_ms", C.c_double), ("partial_bytes", C.c_int64),
                ("n_chunks", C.c_int32), ("n_waves", C.c_int32), ("chunk_cells", C.c_int32), ("slab_snps", C.c_int32), ("n_assigned", C.c_int32),
                ("reserved", C.c_int32 * 3)]


DMX_CLUSTER_LAST_ESTEP = 2


class ClusterMstepRequest(C.Structure):   # dmx_cluster_mstep_request
    _fields_ = [("n_cells", C.c_int32), ("n_snps", C.c_int32), ("n_cols", C.c_int32), ("weights_memory", C.c_int32), ("weights", C.c_void_p),
                ("prior", C.c_void_p), ("floor", C.c_double), ("reserved", C.c_int32 * 4)]


class ClusterEstepRequest(C.Structure):   # dmx_cluster_estep_request
    _fields_ = [("n_restarts", C.c_int32), ("n_clusters", C.c_int32), ("log_pi", C.c_void_p), ("temperature", C.c_double), ("mask", C.c_void_p),
                ("ll", C.c_void_p), ("col_sum", C.c_void_p), ("reserved", C.c_int32 * 4)]


class ClusterInfo(C.Structure):           # dmx_cluster_info
    _fields_ = [("stage_ms", C.c_double), ("mstep_ms", C.c_double), ("estep_ms", C.c_double), ("cache_bytes", C.c_int64), ("scratch_bytes", C.c_int64),
                ("n_pairs", C.c_int64), ("n_cells", C.c_int32), ("n_snps", C.c_int32), ("sorted", C.c_int32), ("n_cols", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class ClusterEstepDoubletRequest(C.Structure):   # dmx_cluster_estep_doublet_request
    _fields_ = [("n_restarts", C.c_int32), ("n_clusters", C.c_int32), ("log_pi", C.c_void_p), ("log_delta", C.c_void_p), ("temperature", C.c_double),
                ("mask", C.c_void_p), ("ll", C.c_void_p), ("col_sum", C.c_void_p), ("dbl_mass", C.c_void_p), ("reserved", C.c_int32 * 4)]


class ClusterDoubletInfo(C.Structure):    # dmx_cluster_doublet_info
    _fields_ = [("doublet_ms", C.c_double), ("estep_ms", C.c_double), ("lld_bytes", C.c_int64), ("n_cells", C.c_int32), ("n_restarts", C.c_int32),
                ("n_clusters", C.c_int32), ("n_pairs", C.c_int32), ("reserved", C.c_int32 * 4)]


class ClusterEstepGroupedRequest(C.Structure):   # dmx_cluster_estep_grouped_request
    _fields_ = [("n_restarts", C.c_int32), ("n_clusters", C.c_int32), ("log_pi", C.c_void_p), ("temperature", C.c_double), ("mask", C.c_void_p),
                ("group", C.c_void_p), ("restarts_per_group", C.c_int32), ("reserved0", C.c_int32), ("ll", C.c_void_p), ("col_sum", C.c_void_p),
                ("reserved", C.c_int32 * 4)]


class ClusterSmInfo(C.Structure):         # dmx_cluster_sm_info
    _fields_ = [("merge_ms", C.c_double), ("grouped_estep_ms", C.c_double), ("n_restarts", C.c_int32), ("n_clusters", C.c_int32),
                ("n_pairs", C.c_int32), ("n_chunks", C.c_int32), ("reserved", C.c_int32 * 4)]


class ClusterHardRequest(C.Structure):    # dmx_cluster_hard_request
    _fields_ = [("n_restarts", C.c_int32), ("n_clusters", C.c_int32), ("doublets", C.c_int32), ("reserved0", C.c_int32), ("active", C.c_void_p),
                ("mask", C.c_void_p), ("label", C.c_void_p), ("n_sing", C.c_void_p), ("n_dbl", C.c_void_p), ("dbl_score", C.c_void_p),
                ("reserved", C.c_int32 * 4)]


class ClusterKInfo(C.Structure):          # dmx_cluster_k_info
    _fields_ = [("evidence_ms", C.c_double), ("hard_ms", C.c_double), ("merge_columns_ms", C.c_double), ("n_restarts", C.c_int32),
                ("n_clusters", C.c_int32), ("n_chunks", C.c_int32), ("n_cells", C.c_int32), ("reserved", C.c_int32 * 4)]


class ClusterEstepKnownRequest(C.Structure):   # dmx_cluster_estep_known_request
    _fields_ = [("n_restarts", C.c_int32), ("n_known", C.c_int32), ("n_free", C.c_int32), ("reserved0", C.c_int32), ("log_pi", C.c_void_p),
                ("temperature", C.c_double), ("mask", C.c_void_p), ("ll", C.c_void_p), ("col_sum", C.c_void_p), ("reserved", C.c_int32 * 4)]


class ClusterMstepWindowRequest(C.Structure):  # dmx_cluster_mstep_window_request
    _fields_ = [("n_cells", C.c_int32), ("n_snps", C.c_int32), ("n_restarts", C.c_int32), ("n_free", C.c_int32), ("weights_memory", C.c_int32),
                ("reserved0", C.c_int32), ("weights", C.c_void_p), ("prior", C.c_void_p), ("floor", C.c_double), ("reserved", C.c_int32 * 4)]


class ClusterKnownInfo(C.Structure):      # dmx_cluster_known_info
    _fields_ = [("estep_ms", C.c_double), ("mstep_ms", C.c_double), ("n_cells", C.c_int32), ("n_known", C.c_int32), ("n_restarts", C.c_int32),
                ("n_free", C.c_int32), ("reserved", C.c_int32 * 4)]


class AmbientRequest(C.Structure):       # dmx_ambient_request
    _fields_ = [("n_cells", C.c_int32), ("assign_memory", C.c_int32), ("assign", C.c_void_p), ("n_snps", C.c_int32), ("n_grid", C.c_int32),
                ("ambient", C.c_void_p), ("grid", C.c_void_p), ("reserved", C.c_int32 * 4)]


class AmbientInfo(C.Structure):          # dmx_ambient_info
    _fields_ = [("kernel_ms", C.c_double), ("profile_bytes", C.c_int64), ("n_cells", C.c_int32), ("n_grid", C.c_int32), ("n_assigned", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class AmbientDoubletRequest(C.Structure):  # dmx_ambient_doublet_request
    _fields_ = [("n_cells", C.c_int32), ("cand_memory", C.c_int32), ("cand", C.c_void_p), ("n_cand", C.c_int32), ("n_alpha", C.c_int32),
                ("n_snps", C.c_int32), ("n_grid", C.c_int32), ("alpha", C.c_void_p), ("ambient", C.c_void_p), ("grid", C.c_void_p),
                ("reserved", C.c_int32 * 4)]


class AmbientDoubletInfo(C.Structure):   # dmx_ambient_doublet_info
    _fields_ = [("kernel_ms", C.c_double), ("profile_bytes", C.c_int64), ("n_used", C.c_int64), ("n_cells", C.c_int32), ("n_cand", C.c_int32),
                ("n_alpha", C.c_int32), ("n_grid", C.c_int32), ("reserved", C.c_int32 * 4)]


class FitRequest(C.Structure):           # dmx_fit_request
    _fields_ = [("n_cells", C.c_int32), ("n_snps", C.c_int32), ("hyp_memory", C.c_int32), ("max_reads", C.c_int32), ("hyp", C.c_void_p),
                ("alpha", C.c_void_p), ("rho", C.c_void_p), ("ambient", C.c_void_p), ("reserved", C.c_int32 * 4)]


class FitInfo(C.Structure):              # dmx_fit_info
    _fields_ = [("kernel_ms", C.c_double), ("bytes", C.c_int64), ("n_trunc", C.c_int64), ("n_zero", C.c_int64), ("n_cells", C.c_int32),
                ("n_used", C.c_int32), ("n_singlet", C.c_int32), ("n_doublet", C.c_int32), ("max_reads", C.c_int32), ("reserved", C.c_int32 * 3)]


class SiteFitRequest(C.Structure):       # dmx_site_fit_request
    _fields_ = [("n_cells", C.c_int32), ("n_snps", C.c_int32), ("hyp_memory", C.c_int32), ("max_reads", C.c_int32), ("hyp", C.c_void_p),
                ("alpha", C.c_void_p), ("rho", C.c_void_p), ("ambient", C.c_void_p), ("partial_bytes", C.c_int64), ("reserved", C.c_int32 * 4)]


class SiteFitInfo(C.Structure):          # dmx_site_fit_info
    _fields_ = [("kernel_ms", C.c_double), ("bytes", C.c_int64), ("partial_bytes", C.c_int64), ("n_trunc", C.c_int64), ("n_zero", C.c_int64),
                ("n_chunks", C.c_int32), ("n_waves", C.c_int32), ("chunk_cells", C.c_int32), ("slab_snps", C.c_int32), ("n_cells", C.c_int32),
                ("n_snps", C.c_int32), ("n_used", C.c_int32), ("n_singlet", C.c_int32), ("n_doublet", C.c_int32), ("max_reads", C.c_int32),
                ("reserved", C.c_int32 * 4)]


DMX_REDRAW_PAIR, DMX_REDRAW_DONOR = 0, 1


class RedrawRequest(C.Structure):        # dmx_redraw_request
    _fields_ = [("n_cells", C.c_int32), ("n_snps", C.c_int32), ("hyp_memory", C.c_int32), ("genotype_draw", C.c_int32), ("hyp", C.c_void_p),
                ("alpha", C.c_void_p), ("rho", C.c_void_p), ("ambient", C.c_void_p), ("seed", C.c_uint64), ("geno_seed", C.c_uint64),
                ("index_base", C.c_int64), ("reserved", C.c_int32 * 4)]


class RedrawInfo(C.Structure):           # dmx_redraw_info
    _fields_ = [("kernel_ms", C.c_double), ("bytes_read", C.c_int64), ("bytes_written", C.c_int64), ("n_pairs_drawn", C.c_int64),
                ("n_pairs_skipped", C.c_int64), ("n_reads_drawn", C.c_int64), ("n_reads_kept", C.c_int64), ("n_cells", C.c_int32),
                ("n_used", C.c_int32), ("n_singlet", C.c_int32), ("n_doublet", C.c_int32), ("genotype_draw", C.c_int32),
                ("reserved", C.c_int32 * 3)]


DMX_KIN_MAX_COLUMNS = 4096


class KinRequest(C.Structure):           # dmx_kin_request
    _fields_ = [("n_snps", C.c_int32), ("n_a", C.c_int32), ("n_b", C.c_int32), ("ga", C.c_void_p), ("gb", C.c_void_p),
                ("weight", C.c_void_p), ("g_memory", C.c_int32), ("reserved", C.c_int32)]


class KinInfo(C.Structure):              # dmx_kin_info
    _fields_ = [("rows_ms", C.c_double), ("tile_ms", C.c_double), ("flop", C.c_int64), ("bytes", C.c_int64), ("n_invalid_a", C.c_int64),
                ("n_invalid_b", C.c_int64), ("n_snps", C.c_int32), ("n_a", C.c_int32), ("n_b", C.c_int32), ("tile_a", C.c_int32),
                ("tile_b", C.c_int32), ("chunk_snps", C.c_int32), ("reserved", C.c_int32 * 2)]


DMX_BLOCK_MAX_EXTRA = 8


class BlockLlkRequest(C.Structure):      # dmx_block_llk_request
    _fields_ = [("n_cells", C.c_int32), ("n_snps", C.c_int32), ("n_blocks", C.c_int32), ("n_extra", C.c_int32), ("block", C.c_void_p),
                ("extra", C.c_void_p), ("extra_memory", C.c_int32), ("reserved", C.c_int32 * 4)]


class InflaterInfo(C.Structure):         # dmx_inflater_info
    _fields_ = [("kernel_ms", C.c_double), ("h2d_ms", C.c_double), ("d2h_ms", C.c_double), ("h2d_bytes", C.c_int64), ("d2h_bytes", C.c_int64),
                ("n_members", C.c_int32), ("n_accepted", C.c_int32), ("n_refused", C.c_int32), ("reserved", C.c_int32 * 3)]


class BlockLlkInfo(C.Structure):         # dmx_block_llk_info
    _fields_ = [("kernel_ms", C.c_double), ("zero_ms", C.c_double), ("result_bytes", C.c_int64), ("n_entries", C.c_int64), ("n_cells", C.c_int32),
                ("n_samples", C.c_int32), ("n_alpha", C.c_int32), ("n_blocks", C.c_int32), ("n_extra", C.c_int32), ("reserved", C.c_int32 * 3)]


DMX_SHARE_INTERIOR, DMX_SHARE_AT_0, DMX_SHARE_AT_1, DMX_SHARE_NOT_CONVERGED, DMX_SHARE_FLAT, DMX_SHARE_NONFINITE = 1, 2, 4, 8, 16, 32


class ShareScanRequest(C.Structure):     # dmx_share_scan_request
    _fields_ = [("n_cells", C.c_int32), ("n_snps", C.c_int32), ("n_anchor", C.c_int32), ("anchor_memory", C.c_int32), ("anchors", C.c_void_p),
                ("rho", C.c_void_p), ("ambient", C.c_void_p), ("reserved", C.c_int32 * 4)]


class ShareFitRequest(C.Structure):      # dmx_share_fit_request
    _fields_ = [("n_cells", C.c_int32), ("n_snps", C.c_int32), ("n_cand", C.c_int32), ("cand_memory", C.c_int32), ("cand", C.c_void_p),
                ("rho", C.c_void_p), ("ambient", C.c_void_p), ("start", C.c_double), ("tol", C.c_double), ("probe", C.c_double),
                ("max_iter", C.c_int32), ("reserved", C.c_int32 * 5)]


class ShareInfo(C.Structure):            # dmx_share_info
    _fields_ = [("scan_ms", C.c_double), ("fit_ms", C.c_double), ("scan_bytes", C.c_int64), ("fit_bytes", C.c_int64), ("scan_entries", C.c_int64),
                ("fit_used", C.c_int64), ("fit_evals", C.c_int64), ("n_cells", C.c_int32), ("n_samples", C.c_int32), ("n_anchor", C.c_int32),
                ("n_cand", C.c_int32), ("have_scan", C.c_int32), ("have_fit", C.c_int32), ("reserved", C.c_int32 * 4)]


class TripletRequest(C.Structure):     # dmx_triplet_request
    _fields_ = [("n_cells", C.c_int32), ("base_memory", C.c_int32), ("base", C.c_void_p), ("n_base", C.c_int32), ("n_shares", C.c_int32),
                ("n_snps", C.c_int32), ("reserved0", C.c_int32), ("shares", C.c_void_p), ("reserved", C.c_int32 * 4)]


class TripletInfo(C.Structure):        # dmx_triplet_info
    _fields_ = [("kernel_ms", C.c_double), ("profile_bytes", C.c_int64), ("n_used", C.c_int64), ("n_cells", C.c_int32), ("n_base", C.c_int32),
                ("n_shares", C.c_int32), ("n_samples", C.c_int32), ("reserved", C.c_int32 * 4)]


class AnchoredRequest(C.Structure):    # dmx_anchored_request
    _fields_ = [("n_cells", C.c_int32), ("n_anchor", C.c_int32), ("anchor_memory", C.c_int32), ("reserved0", C.c_int32), ("anchors", C.c_void_p),
                ("reserved", C.c_int32 * 4)]


class AnchoredInfo(C.Structure):       # dmx_anchored_info
    _fields_ = [("col_ms", C.c_double), ("pair_ms", C.c_double), ("reduce_ms", C.c_double), ("result_bytes", C.c_int64), ("n_entries", C.c_int64),
                ("n_cells", C.c_int32), ("n_samples", C.c_int32), ("n_alpha", C.c_int32), ("n_anchor", C.c_int32), ("reserved", C.c_int32 * 4)]


class ComposeRequest(C.Structure):     # dmx_compose_request
    _fields_ = [("n_out", C.c_int32), ("reserved0", C.c_int32), ("index_base", C.c_int64), ("parent", C.c_void_p), ("keep", C.c_void_p),
                ("seed", C.c_uint64), ("reserved", C.c_int32 * 4)]


class ComposeInfo(C.Structure):        # dmx_compose_info
    _fields_ = [("n_pairs", C.c_int64), ("n_reads", C.c_int64), ("bytes_read", C.c_int64), ("bytes_written", C.c_int64),
                ("count_ms", C.c_double), ("scan_ms", C.c_double), ("fill_ms", C.c_double), ("n_out", C.c_int32), ("nrd_width", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class PriorRequest(C.Structure):       # dmx_prior_request
    _fields_ = [("n_cells", C.c_int32), ("n_samples", C.c_int32), ("n_alpha", C.c_int32), ("grid_memory", C.c_int32), ("grid", C.c_void_p),
                ("mask", C.c_void_p), ("pi0", C.c_void_p), ("d0", C.c_double), ("tol", C.c_double), ("max_iter", C.c_int32),
                ("fix_pi", C.c_int32), ("fix_d", C.c_int32), ("reserved", C.c_int32 * 5)]


class PriorCall(C.Structure):          # dmx_prior_call
    _fields_ = [("log_e", C.c_double), ("p_sng", C.c_double), ("p_het", C.c_double), ("p_hom", C.c_double), ("p_sng1", C.c_double),
                ("p_sng2", C.c_double), ("p_dbl1", C.c_double), ("i_sng1", C.c_int32), ("i_sng2", C.c_int32), ("j_dbl", C.c_int32),
                ("k_dbl", C.c_int32), ("n_dbl", C.c_int32), ("flag", C.c_int32)]


PRIOR_CALL_DTYPE = np.dtype([(n, np.float64 if t is C.c_double else np.int32) for n, t in PriorCall._fields_])


class PriorInfo(C.Structure):          # dmx_prior_info
    _fields_ = [("estep_ms", C.c_double), ("fold_ms", C.c_double), ("call_ms", C.c_double), ("fit_ms", C.c_double),
                ("bytes_per_iter", C.c_int64), ("n_iter", C.c_int32), ("n_cells", C.c_int32), ("n_samples", C.c_int32), ("n_alpha", C.c_int32),
                ("waves_per_block", C.c_int32), ("reserved", C.c_int32 * 3)]


class CensusStepRequest(C.Structure):  # dmx_census_step_request
    _fields_ = [("n_cells", C.c_int32), ("group_memory", C.c_int32), ("group", C.c_void_p), ("n_groups", C.c_int32), ("n_samples", C.c_int32),
                ("w", C.c_void_p), ("acc", C.c_void_p), ("ll", C.c_void_p), ("gap", C.c_void_p), ("n_read", C.c_void_p), ("n_pair", C.c_void_p),
                ("reserved", C.c_int32 * 4)]


class CensusRequest(C.Structure):      # dmx_census_request
    _fields_ = [("n_cells", C.c_int32), ("group_memory", C.c_int32), ("group", C.c_void_p), ("n_groups", C.c_int32), ("n_samples", C.c_int32),
                ("w0", C.c_void_p), ("tol", C.c_double), ("max_steps", C.c_int32), ("accelerate", C.c_int32), ("reserved", C.c_int32 * 4)]


class CensusInfo(C.Structure):         # dmx_census_info
    _fields_ = [("kernel_ms", C.c_double), ("dosage_ms", C.c_double), ("dosage_bytes", C.c_int64), ("partial_bytes", C.c_int64),
                ("n_steps", C.c_int32), ("n_invalid_snps", C.c_int32), ("n_groups", C.c_int32), ("n_chunks", C.c_int32), ("n_cells", C.c_int32),
                ("n_samples", C.c_int32), ("reserved", C.c_int32 * 4)]


class CensusFisherRequest(C.Structure):  # dmx_census_fisher_request
    _fields_ = [("n_cells", C.c_int32), ("group_memory", C.c_int32), ("group", C.c_void_p), ("n_groups", C.c_int32), ("n_samples", C.c_int32),
                ("w", C.c_void_p), ("H", C.c_void_p), ("score", C.c_void_p), ("n_read_b", C.c_void_p), ("acc", C.c_void_p), ("ll", C.c_void_p),
                ("n_read", C.c_void_p), ("n_pair", C.c_void_p), ("reserved", C.c_int32 * 4)]


class CensusFisherInfo(C.Structure):     # dmx_census_fisher_info
    _fields_ = [("kernel_ms", C.c_double), ("partial_bytes", C.c_int64), ("n_groups", C.c_int32), ("n_chunks", C.c_int32),
                ("n_blocks", C.c_int32), ("n_entries", C.c_int32), ("n_cells", C.c_int32), ("n_samples", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class DmxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libdmx error {code}: {msg}")
        self.code = code


class Pileup(C.Structure):
    _fields_ = [("n_cells", C.c_int32), ("n_snps", C.c_int32), ("n_pairs", C.c_int64), ("n_reads", C.c_int64),
                ("cell_pair_off", C.c_void_p), ("cell_read_off", C.c_void_p), ("pair_snp", C.c_void_p),
                ("pair_nrd", C.c_void_p), ("nrd_width", C.c_int32), ("memory", C.c_int32), ("reads", C.c_void_p),
                ("rd_totl", C.c_void_p), ("rd_pass", C.c_void_p), ("rd_uniq", C.c_void_p)]


class EngineConfig(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("n_alpha", C.c_int32), ("alpha", C.c_void_p), ("doublet_prior", C.c_double),
                ("device", C.c_int32), ("mode", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class CellSummary(C.Structure):
    _fields_ = [("max_llk", C.c_double), ("sum_single", C.c_double), ("sum_double", C.c_double),
                ("sing_llk1", C.c_double), ("sing_llk2", C.c_double),
                ("llk12", C.c_double), ("llk1", C.c_double), ("llk2", C.c_double), ("llk10", C.c_double), ("llk20", C.c_double),
                ("llk00_0", C.c_double), ("llk00_best", C.c_double),
                ("i_sing1", C.c_int32), ("i_sing2", C.c_int32), ("j_best", C.c_int32), ("k_best", C.c_int32),
                ("n_best", C.c_int32), ("n_pairs", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
                ("llk_ab", C.c_double), ("llk_ba", C.c_double), ("llk_ab_alt", C.c_double), ("llk_ba_alt", C.c_double),
                ("ev_x_ab", C.c_double), ("ev_t_ab", C.c_double), ("ev_x_ba", C.c_double), ("ev_t_ba", C.c_double)]


SUMMARY_DTYPE = np.dtype([(n, np.float64) for n in ("max_llk", "sum_single", "sum_double", "sing_llk1", "sing_llk2", "llk12",
                                                    "llk1", "llk2", "llk10", "llk20", "llk00_0", "llk00_best")] +
                         [(n, np.int32) for n in ("i_sing1", "i_sing2", "j_best", "k_best", "n_best", "n_pairs", "flags", "reserved")] +
                         [(n, np.float64) for n in ("llk_ab", "llk_ba", "llk_ab_alt", "llk_ba_alt", "ev_x_ab", "ev_t_ab", "ev_x_ba", "ev_t_ba")])
assert SUMMARY_DTYPE.itemsize == C.sizeof(CellSummary)


class DeviceView(C.Structure):
    _fields_ = [("llks", C.c_void_p), ("llk0s", C.c_void_p), ("llksAB", C.c_void_p), ("llks00", C.c_void_p),
                ("summary", C.c_void_p), ("gp0s", C.c_void_p), ("sing", C.c_void_p)]


class KernelTimes(C.Structure):
    _fields_ = [("gp0_ms", C.c_float), ("singlet_ms", C.c_float), ("doublet_ms", C.c_float), ("reduce_ms", C.c_float)]


class KernelTimeMeans(C.Structure):
    _fields_ = [("singlet_ms", C.c_double), ("doublet_ms", C.c_double), ("reduce_ms", C.c_double), ("certify_ms", C.c_double),
                ("n_singlet", C.c_int32), ("n_doublet", C.c_int32)]


class KernelNames(C.Structure):
    _fields_ = [("singlet", C.c_char * 96), ("doublet", C.c_char * 96), ("certify", C.c_char * 96), ("k1_placement", C.c_int32), ("reserved", C.c_int32 * 3)]


class KernelBytes(C.Structure):
    _fields_ = [("singlet_bytes", C.c_double), ("doublet_bytes", C.c_double), ("reduce_bytes", C.c_double)]


class FinalInput(C.Structure):
    _fields_ = [("n_cells", C.c_int32), ("n_samples", C.c_int32), ("n_alpha", C.c_int32), ("alpha", C.c_void_p),
                ("doublet_prior", C.c_double), ("min_total", C.c_int32), ("min_uniq", C.c_int32), ("min_snp", C.c_int32),
                ("write_pair", C.c_int32), ("barcodes", C.c_void_p), ("sample_ids", C.c_void_p),
                ("rd_totl", C.c_void_p), ("rd_pass", C.c_void_p), ("rd_uniq", C.c_void_p), ("n_snp", C.c_void_p),
                ("llks", C.c_void_p), ("llk0s", C.c_void_p), ("llksAB", C.c_void_p), ("llks00", C.c_void_p),
                ("tie_pileup", C.c_void_p), ("tie_g", C.c_void_p), ("tie_tol", C.c_double)]


class Job(C.Structure):
    _fields_ = [("store", C.c_void_p), ("g", C.c_void_p), ("n_samples", C.c_int32), ("sample_ids", C.c_void_p),
                ("n_alpha", C.c_int32), ("alpha", C.c_void_p), ("doublet_prior", C.c_double),
                ("min_total", C.c_int32), ("min_uniq", C.c_int32), ("min_snp", C.c_int32), ("write_pair", C.c_int32),
                ("out_prefix", C.c_char_p), ("device", C.c_int32), ("arbiter", C.c_int32), ("n_gpus", C.c_int32), ("mode", C.c_int32),
                ("pileup", C.c_void_p), ("barcodes", C.c_void_p), ("timing", C.c_void_p)]


class JobTiming(C.Structure):
    _fields_ = [("freeze_s", C.c_double), ("setup_s", C.c_double), ("stage_s", C.c_double), ("wait_s", C.c_double),
                ("write_s", C.c_double), ("total_s", C.c_double), ("kernel_ms", C.c_double),
                ("n_ranges", C.c_int32), ("n_engines", C.c_int32), ("n_cells_grid_fetched", C.c_int32), ("n_cells_single", C.c_int32)]


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen libdmx.so; fails loudly when it has not been built (python -m demuxlet_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # torch bundles its own libamdhip64 (same SONAME as /opt/rocm's).  Load torch FIRST so that libdmx.so binds to
        # that copy: two HIP runtimes in one process leave whichever comes second without a device.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not LIB_PATH.exists():
        raise DmxError(-100, f"{LIB_PATH} is missing — build it with `python -m demuxlet_amd.build` (hipcc, gfx950)")
    L = C.CDLL(str(LIB_PATH))
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.dmx_abi_version.restype = C.c_int
    L.dmx_last_error.restype = C.c_char_p
    sig = {
        "dmx_device_warm_up": [i32, i32], "dmx_phred_tables": [vp, vp], "dmx_geno_from_gt": [vp, i32, dbl, vp], "dmx_geno_from_pl": [vp, i32, vp],
        "dmx_geno_from_gp": [vp, i32, dbl, vp], "dmx_store_free": [vp], "dmx_store_add_snp": [vp],
        "dmx_store_add_cell": [vp, C.c_char_p], "dmx_store_count_read": [vp, i32],
        "dmx_store_add_read": [vp, i32, i32, C.c_char_p, i32, i32], "dmx_store_n_cells": [vp], "dmx_store_n_snps": [vp],
        "dmx_store_barcode": [vp, i32], "dmx_store_freeze": [vp, vp], "dmx_engine_create": [vp, vp],
        "dmx_engine_destroy": [vp], "dmx_engine_set_stream": [vp, vp], "dmx_engine_set_phred_tables": [vp, vp, vp],
        "dmx_engine_set_genotypes": [vp, vp, i32, i32], "dmx_engine_set_pileup": [vp, vp], "dmx_engine_run_singlet": [vp],
        "dmx_engine_run_doublet": [vp], "dmx_engine_run": [vp], "dmx_engine_sync": [vp], "dmx_engine_get_singlet": [vp, vp, vp],
        "dmx_engine_get_doublet": [vp, vp, vp, vp], "dmx_engine_device_view": [vp, vp],
        "dmx_engine_last_kernel_times": [vp, vp], "dmx_engine_algorithmic_bytes": [vp, vp],
        "dmx_write_single": [vp, C.c_char_p], "dmx_write_doublet": [vp, C.c_char_p], "dmx_demuxlet_run": [vp],
        "dmx_debug_device_log": [vp, vp, C.c_int64, i32], "dmx_debug_device_log2": [vp, vp, C.c_int64, i32], "dmx_debug_device_log2_lite": [vp, vp, C.c_int64, i32], "dmx_debug_device_log2_lite32": [vp, vp, C.c_int64, i32],
        "dmx_debug_device_log2_mirror": [vp, vp, vp, vp, C.c_int64, i32],
        "dmx_engine_get_sing": [vp, vp], "dmx_write_doublet_summary": [vp, vp, vp, C.c_char_p],
        "dmx_debug_device_div": [vp, vp, vp, C.c_int64, i32],
        "dmx_debug_log_rate": [i32, i32, i32, vp],
        "dmx_engine_get_cell_grids": [vp, vp, i32, vp],
        "dmx_debug_log_dd": [vp, vp, vp, vp, vp, C.c_int64],
        "dmx_resolve_tie_order": [vp, C.c_int64],
        "dmx_engine_mean_kernel_times": [vp, i32, vp],
        "dmx_store_add_batch": [vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, i32],
        "dmx_write_doublet_summary_grids": [vp, vp, vp, vp, C.c_char_p],
        "dmx_engine_kernel_names": [vp, vp],
        "dmx_engine_format_pair": [vp, vp, vp], "dmx_pair_text_get_info": [vp, vp], "dmx_pair_text_get_scalars": [vp, vp], "dmx_pair_text_read": [vp, C.c_int64, C.c_int64, vp],
        "dmx_engine_refine_genotypes": [vp, vp], "dmx_engine_get_refined": [vp, vp, vp, vp, vp, vp], "dmx_engine_refined_device_ptr": [vp, vp],
        "dmx_engine_refine_info": [vp, vp],
        "dmx_engine_cluster_stage": [vp], "dmx_engine_cluster_mstep": [vp, vp], "dmx_engine_cluster_estep": [vp, vp],
        "dmx_engine_get_cluster": [vp, vp, vp, vp, vp], "dmx_engine_get_cluster_stage": [vp, vp, vp, vp, vp], "dmx_engine_cluster_device_ptr": [vp, vp],
        "dmx_engine_cluster_info": [vp, vp],
        "dmx_engine_cluster_doublet": [vp, i32, i32], "dmx_engine_get_cluster_doublet": [vp, vp, vp], "dmx_engine_cluster_estep_doublet": [vp, vp],
        "dmx_engine_cluster_doublet_info": [vp, vp],
        "dmx_engine_cluster_merge_score": [vp, i32, i32, vp, C.c_double, vp, vp], "dmx_engine_cluster_estep_grouped": [vp, vp],
        "dmx_engine_cluster_sm_info": [vp, vp],
        "dmx_engine_cluster_evidence": [vp, i32, i32, vp, C.c_double, vp, vp], "dmx_engine_cluster_hard": [vp, vp],
        "dmx_engine_get_cluster_hard": [vp, vp, vp, vp, vp],
        "dmx_engine_cluster_hard_device_ptr": [vp, vp], "dmx_engine_cluster_merge_columns": [vp, i32, i32, vp, vp],
        "dmx_engine_cluster_k_info": [vp, vp],
        "dmx_engine_cluster_set_known": [vp, i32, i32, vp, i32], "dmx_engine_cluster_estep_known": [vp, vp],
        "dmx_engine_cluster_mstep_window": [vp, vp], "dmx_engine_get_cluster_known": [vp, vp], "dmx_engine_cluster_known_info": [vp, vp],
        "dmx_engine_ambient": [vp, vp], "dmx_engine_get_ambient": [vp, vp, vp, vp], "dmx_engine_ambient_info": [vp, vp],
        "dmx_engine_ambient_doublet": [vp, vp], "dmx_engine_get_ambient_doublet": [vp, vp, vp, vp], "dmx_engine_ambient_doublet_info": [vp, vp],
        "dmx_engine_doublet_anchored": [vp, vp], "dmx_engine_get_anchored": [vp, vp, vp, vp, vp, vp], "dmx_engine_anchored_info": [vp, vp],
        "dmx_engine_triplet": [vp, vp], "dmx_engine_get_triplet": [vp, vp, vp, vp], "dmx_engine_triplet_info": [vp, vp],
        "dmx_engine_compose": [vp, vp], "dmx_engine_composed_pileup": [vp, vp], "dmx_engine_get_composed": [vp, vp, vp, vp, vp, vp],
        "dmx_engine_compose_info": [vp, vp],
        "dmx_engine_census_step": [vp, vp], "dmx_engine_census": [vp, vp], "dmx_engine_get_census": [vp, vp, vp, vp, vp, vp, vp, vp],
        "dmx_engine_census_info": [vp, vp],
        "dmx_engine_census_fisher": [vp, vp], "dmx_engine_census_fisher_info": [vp, vp],
        "dmx_engine_prior_step": [vp, vp, vp, dbl], "dmx_engine_get_prior_step": [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "dmx_engine_prior_fit": [vp, vp], "dmx_engine_get_prior_fit": [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32],
        "dmx_engine_prior_call": [vp, vp, vp, dbl], "dmx_engine_get_prior_calls": [vp, vp], "dmx_engine_prior_info": [vp, vp],
        "dmx_engine_fit": [vp, vp], "dmx_engine_get_fit": [vp, vp, vp, vp, vp, vp, vp, vp], "dmx_engine_fit_info": [vp, vp],
        "dmx_engine_share_scan": [vp, vp], "dmx_engine_get_share_scan": [vp, vp, vp], "dmx_engine_share_fit": [vp, vp],
        "dmx_engine_get_share_fit": [vp, vp, vp], "dmx_engine_share_info": [vp, vp],
        "dmx_engine_site_fit": [vp, vp], "dmx_engine_get_site_fit": [vp] * 11, "dmx_engine_site_fit_info": [vp, vp],
        "dmx_engine_redraw": [vp, vp], "dmx_engine_redrawn_pileup": [vp, vp], "dmx_engine_get_redrawn": [vp, vp, vp],
        "dmx_engine_redraw_info": [vp, vp],
        "dmx_engine_geno_compare": [vp, vp], "dmx_engine_get_geno_compare": [vp, vp, vp, vp], "dmx_engine_geno_compare_info": [vp, vp],
        "dmx_engine_block_llk": [vp, vp], "dmx_engine_get_block_llk": [vp, vp, vp, vp, vp], "dmx_engine_block_llk_info": [vp, vp],
        "dmx_inflater_create": [i32, i32, i64, i64, vp], "dmx_inflater_free": [vp],
        "dmx_inflater_submit": [vp, i32, i32, vp, vp, vp, vp, vp, vp], "dmx_inflater_wait": [vp, i32, vp, vp],
        "dmx_inflater_run": [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp], "dmx_inflater_pin": [vp, i64], "dmx_inflater_unpin": [vp],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = C.c_int
    L.dmx_store_new.restype = vp
    L.dmx_store_new.argtypes = []
    L.dmx_store_free.restype = None
    L.dmx_store_barcode.restype = C.c_char_p
    L.dmx_pair_text_free.restype = None
    L.dmx_pair_text_free.argtypes = [vp]
    _lib = L
    return L


def check(rc: int) -> int:
    if rc < 0:
        raise DmxError(rc, load().dmx_last_error().decode(errors="replace"))
    return rc
