/* dmx.h — C-ABI of libdmx, the MI355X-native (gfx950, HIP) replacement for demuxlet's per-barcode
 * genotype-likelihood engine.
 *
 * The reference (statgen/demuxlet) has no plugin/FFI interface: the engine is inline in main()
 * (cmd_cram_demuxlet.cpp:390-881) between two in-memory cuts:
 *     B1  after the BAM x VCF scan:  sc_dropseq_lib_t scl (sc_drop_seq.h:34-58) + per-SNP genotype probabilities
 *     B2  before the text writers:   llks[B][V], llk0s[B], llksAB[V][V][A] per cell, llks00[A] per cell
 * This header IS that boundary.  Every entry point names the reference lines it replaces.  A maintainer keeps
 * cmd_cram_demuxlet.cpp:1-388 (options, htslib scan) and replaces :390-881 by the calls shown in INTEGRATION.md.
 *
 * Conventions: plain C, plain pointers and sizes, no C++/torch types.  Every function returns DMX_OK (0) or a negative
 * dmx_status; dmx_last_error() gives the message of the last failure on the calling thread.  The library never exits
 * or throws across the ABI (the reference's error() prints and throws, Error.cpp:27-41; the caller decides).
 * Handles are not thread-safe; one engine drives one GPU on one HIP stream.  There is NO CPU fallback: engine entry
 * points fail with DMX_ERR_NOGPU / DMX_ERR_HIP when no gfx950 device is usable.
 */
#ifndef DMX_H
#define DMX_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DMX_ABI_VERSION 8   /* 4: dmx_store_add_batch, dmx_engine_mean_kernel_times; 5: dmx_device_warm_up, dmx_engine_run; 6: dmx_engine_get_cell_grids;
                               7: DMX_CELL_NEAR_RULE, dmx_write_doublet_summary_grids, dmx_engine_kernel_names, dmx_debug_device_log2_lite.  ABI 6 had grown dmx_final_input in place by a
                               trailing `cell_grid` member; a by-pointer input struct without a size member cannot grow (a caller compiled against ABI 5
                               passes a shorter object), so ABI 7 WITHDRAWS that member — the struct has its ABI 5 layout again and the grids travel as an
                               argument of the new entry point.  Additions only otherwise: callers of ABI <= 5 run unchanged.
                               8: dmx_engine_format_pair / dmx_pair_text_* (`.pair` rows formatted on the device); later, still ABI 8:
                               dmx_engine_refine_genotypes / _get_refined / _refined_device_ptr / _refine_info (genotype refinement from
                               called singlets); dmx_engine_cluster_* (genotype-free clustering); dmx_engine_ambient / _get_ambient /
                               _ambient_info (per-barcode ambient contamination profile); dmx_engine_cluster_doublet / _get_cluster_doublet /
                               _cluster_estep_doublet / _cluster_doublet_info (doublet-aware clustering); dmx_engine_cluster_merge_score /
                               _cluster_estep_grouped / _cluster_sm_info (split-merge moves); dmx_engine_cluster_set_known /
                               _cluster_estep_known / _cluster_mstep_window / _get_cluster_known / _cluster_known_info (partly
                               genotyped pools); dmx_engine_ambient_doublet / _get_ambient_doublet / _ambient_doublet_info (doublet
                               likelihood with a soup term, to tell soupy singlets from doublets); dmx_engine_triplet / _get_triplet /
                               _triplet_info (a base pair with every sample as a third donor); dmx_engine_cluster_evidence /
                               _cluster_hard / _get_cluster_hard / _cluster_hard_device_ptr / _cluster_merge_columns / _cluster_k_info (choosing the number
                               of clusters); dmx_engine_compose / _composed_pileup / _get_composed / _compose_info (barcodes composed on
                               the device from other barcodes' reads); dmx_engine_doublet_anchored / _get_anchored / _anchored_info
                               (the doublet search over each barcode's best singlets as anchors: wide panels without the V x V grid);
                               dmx_engine_fit / _get_fit / _fit_info (goodness of fit of each barcode's hypothesis);
                               dmx_engine_share_scan / _get_share_scan / _share_fit / _get_share_fit / _share_info (every partner of a
                               barcode's anchors scored at alpha = 0, and a doublet's mixing share fitted continuously);
                               dmx_engine_site_fit / _get_site_fit / _site_fit_info (goodness of fit of each SNP's row);
                               dmx_engine_redraw / _redrawn_pileup / _get_redrawn / _redraw_info (every read's allele drawn again
                               from the model: the staged pool's null pool); dmx_engine_block_llk / _get_block_llk /
                               _block_llk_info (singlet column, llks00 and chosen grid entries summed per genomic block);
                               dmx_inflater_create / _free / _submit / _wait / _run / _pin / _unpin (BGZF members inflated on the
                               device, for the scanner's opt-in DMX_GPU_INFLATE stage).
                               Additions only. */

typedef enum {
  DMX_OK = 0,
  DMX_ERR_ARG = -1,      /* bad argument / precondition (e.g. n_samples < 2 for the doublet stage, cmd_cram_demuxlet.cpp:731,:821) */
  DMX_ERR_HIP = -2,      /* a HIP runtime call failed */
  DMX_ERR_STATE = -3,    /* call order (e.g. run before set_pileup) */
  DMX_ERR_IO = -4,       /* cannot create an output file (cmd_cram_demuxlet.cpp:409-410,:535-536) */
  DMX_ERR_NOGPU = -5,    /* no usable gfx950 device */
  DMX_ERR_NOMEM = -6
} dmx_status;

enum { DMX_MEM_HOST = 0, DMX_MEM_DEVICE = 1 };

int         dmx_abi_version(void);
const char* dmx_last_error(void);

/* ------------------------------------------------------------------------------------------------------------------
 * a2  phred LUT — replaces the global phredConv (PhredHelper.cpp:24-40): err[q] = q>1 ? pow(0.1, q*0.1) : 0.75,
 *     mat[q] = 1-err[q].  Computed with the HOST libm so that the device uses the very doubles the reference would. */
int dmx_phred_tables(double mat[256], double err[256]);

/* ------------------------------------------------------------------------------------------------------------------
 * a3  genotype FORMAT field -> float32 probability triplets (replaces BCFFilteredReader::parse_posteriors,
 *     bcf_filtered_reader.cpp:360-454, parse_genotypes :186-242, parse_likelihoods :244-320) for one biallelic,
 *     diploid record.  Inputs are the raw htslib arrays restricted to the selected samples:
 *       alleles[2*i+h]  allele index (bcf_gt_allele) of haplotype h, or -1 when missing
 *       pl[3*i+g]       PL integers (INT32_MIN = bcf_int32_missing)
 *       gp[3*i+g]       GP floats
 *     out[3*i+g] is what get_posterior_at(3*i+g) would return (bcf_filtered_reader.h:159-161). */
int dmx_geno_from_gt(const int32_t* alleles, int32_t n_samples, double gt_error, float* out);
int dmx_geno_from_pl(const int32_t* pl, int32_t n_samples, float* out);      /* --geno-error is not used on the PL path */
int dmx_geno_from_gp(const float* gp, int32_t n_samples, double gt_error, float* out);

/* ------------------------------------------------------------------------------------------------------------------
 * a1  UMI-deduplicated pileup store — replaces sc_dropseq_lib_t (sc_drop_seq.h:34-58, sc_drop_seq.cpp:3-77).
 *     Same call sequence as the reference's scan loop: add_snp per VCF record (:184,:231), add_cell per read (:262),
 *     count_read per read (:295 ++cell_totl_reads), add_read per (read, overlapping SNP) (:325).
 *     add_read returns 1 when the (snp,cell,umi) key is new (first observation wins), 0 for a duplicate
 *     (sc_drop_seq.cpp:44,53,57), <0 on error. */
typedef struct dmx_store dmx_store;
dmx_store* dmx_store_new(void);
void       dmx_store_free(dmx_store*);
int32_t    dmx_store_add_snp(dmx_store*);                              /* returns the new snp id */
int32_t    dmx_store_add_cell(dmx_store*, const char* barcode);        /* returns the (new or existing) cell id */
int        dmx_store_count_read(dmx_store*, int32_t cell);
int        dmx_store_add_read(dmx_store*, int32_t snp, int32_t cell, const char* umi, int32_t allele, int32_t bq);
/* n dmx_store_add_read calls in the order given (item i: snp[i], cell[i], the umi_len[i] bytes at umi_pool + umi_off[i], allele[i],
 * bq[i]); is_new[i] (optional) receives what the i-th call would have returned.  Observations of different cells are inserted on up to
 * n_threads host threads (0 = all): a (snp, cell, umi) key lives in one cell shard, and inside a shard the given order is kept, which is
 * all that "first observation wins" can see — the store ends up exactly as after the n single calls.  Used by the `demuxlet` binary's
 * scan, which overlaps reads and SNPs on all host cores and hands the observations over window by window, in BAM order. */
int        dmx_store_add_batch(dmx_store*, int64_t n, const int32_t* snp, const int32_t* cell, const char* umi_pool, const uint64_t* umi_off,
                               const uint32_t* umi_len, const uint8_t* allele, const uint8_t* bq, uint8_t* is_new, int32_t n_threads);
int32_t    dmx_store_n_cells(const dmx_store*);
int32_t    dmx_store_n_snps(const dmx_store*);
const char* dmx_store_barcode(const dmx_store*, int32_t cell);

/* The pileup in the layout the GPU consumes (SoA/CSR).  Cells are in id order; a cell's pairs are in ascending SNP id
 * (iteration order of std::map<int32_t,...>, cmd_cram_demuxlet.cpp:595); a pair's reads are in ascending UMI byte
 * order (std::map<std::string,...>, :428,:600) because the per-read renormalisation makes that order observable.
 * Reads with allele 2 ("neither REF nor ALT") are not stored: both likelihood loops skip them (:435,:604); they still
 * create their pair (N.SNP) and count in the read counters. */
typedef struct {
  int32_t  n_cells, n_snps;
  int64_t  n_pairs, n_reads;
  const int64_t* cell_pair_off;   /* [n_cells+1] first pair of each cell */
  const int64_t* cell_read_off;   /* [n_cells+1] first read byte of each cell */
  const int32_t* pair_snp;        /* [n_pairs] SNP id, or NULL = dense layout (every cell has n_snps pairs, pair t is SNP t) */
  const void*    pair_nrd;        /* [n_pairs] stored reads of the pair, nrd_width bytes each */
  int32_t        nrd_width;       /* 1, 2 or 4 */
  int32_t        memory;          /* DMX_MEM_HOST or DMX_MEM_DEVICE — where ALL the arrays above and below live */
  const uint8_t* reads;           /* [n_reads] (allele<<7)|bq, allele in {0,1}, bq <= 127 */
  /* per-cell counters of the pileup stage; host memory always; only the finaliser reads them (may be NULL for dmx_engine_*) */
  const int32_t *rd_totl, *rd_pass, *rd_uniq;   /* RD.TOTL (:295) RD.PASS (sc_drop_seq.cpp:39) RD.UNIQ (:75) */
} dmx_pileup;

/* Freeze the store into a dmx_pileup (host memory, owned by the store, valid until the next add_* or free). */
int dmx_store_freeze(dmx_store*, dmx_pileup* out);

/* ------------------------------------------------------------------------------------------------------------------
 * a4,a5,a7,a8,a9,a10  the likelihood engine on one MI355X — replaces cmd_cram_demuxlet.cpp:390-401 (gp0s), :412-461
 *     (singlet accumulation), :542-560 (pair tables, never materialised) and :576-734 (doublet grid + per-cell sums). */
typedef struct dmx_engine dmx_engine;

typedef struct {
  int32_t n_samples;           /* V  = vr.get_nsamples() */
  int32_t n_alpha;             /* A  = gridAlpha.size(); alpha[0] is the singlet entry whatever its value (:726,:730) */
  const double* alpha;         /* [A] */
  double  doublet_prior;       /* --doublet-prior */
  int32_t device;              /* HIP device ordinal */
  int32_t mode;                /* DMX_MODE_STRICT (0): reference operation order, no FMA contraction, IEEE division; or DMX_MODE_FAST */
  int32_t flags;               /* DMX_ENGINE_* */
  int32_t reserved[3];
} dmx_engine_config;
enum { DMX_MODE_STRICT = 0,
       /* Same ownership and accumulation order as STRICT.  Inside a doublet term the nine-term sum of cmd_cram_demuxlet.cpp:677-679
        * is factored as g_j . (pG[n] g_k) with fused multiply-adds, and for the default grid {0, 0.5} only the
        * entries demuxlet prints or decides on are evaluated: llksAB[j][0][0] and one of llksAB[j][k][1] / [k][j][1] (mirrored);
        * llksAB[j][k != 0][0], read by the maxLLK scan (:713-721) only, is filled with llksAB[j][0][0].
        * A printed log-likelihood moves by <= ~6e-11 (tests bound it by 1e-9 against the reference); .best stays identical.
        * Other alpha grids that start with 0 (`--alpha` is multi-valued, cmd_cram_demuxlet.cpp:57) evaluate the singlet column and every
        * (j, k) of the alphas n >= 1 in the same bilinear form (soft fields, up to 128 samples); GT inputs with such grids, grids with
        * alpha[0] != 0 and wider panels (soft fields: 512 samples on the default grid, 128 on the others; GT inputs: 64) run the STRICT kernels,
        * whose results FAST's contract includes. */
       DMX_MODE_FAST = 1 };
enum { DMX_ENGINE_NO_CERTIFY = 1   /* skip the device-side tie-order certificate (K3b): for callers that do not need the
                                      reference's DBL-a-b / DBL-b-a order (dmx_job.arbiter = 0 sets it) */ };

/* per-cell result of the device-side reduction (K3) — what :713-734 and :746-770,:799-828 derive from one cell's grid */
typedef struct {
  double  max_llk;             /* :713-721 */
  double  sum_single;          /* :726 */
  double  sum_double;          /* :728-733 */
  double  sing_llk1, sing_llk2;/* llksAB[iSing1][0][0], llksAB[iSing2][0][0]  (:816-817) */
  double  llk12, llk1, llk2, llk10, llk20;   /* :820-825 */
  double  llk00_0, llk00_best; /* llks00[0] (:819), llks00[alphaBest] (:826) */
  int32_t i_sing1, i_sing2;    /* :746-758 (first maximum wins; second = first maximum of the rest) */
  int32_t j_best, k_best, n_best;            /* :799-814 (strict <: lowest (j,k,n) scan index among equal maxima) */
  int32_t n_pairs;             /* N.SNP of the cell; 0 => the cell has no .best row (:592) */
  int32_t flags;               /* DMX_CELL_* : decisions that sit within 1e-7 of an alternative other than the (j,k)/(k,j) mirror */
  int32_t reserved;
  double  llk_ab, llk_ba;      /* with DMX_CELL_ORDER_CERTIFIED: llksAB[a][b][n_best] and llksAB[b][a][n_best], a = min(j_best, k_best),
                                  b = max, exactly as the reference computes them (what the host tie arbiter would re-evaluate) */
  /* with DMX_CELL_ORDER_RESOLVABLE: each accumulator is one of two known doubles, and which one hangs on what the reference's
   * libm returns for ONE log():  llksAB[a][b] = llk_ab if log(ev_x_ab) == ev_t_ab, llk_ab_alt if it is the next double above
   * ev_t_ab (anything else: no statement); likewise (b,a).  An accumulator with llk_*_alt == llk_* is already certain. */
  double  llk_ab_alt, llk_ba_alt;
  double  ev_x_ab, ev_t_ab, ev_x_ba, ev_t_ba;
} dmx_cell_summary;
enum { DMX_CELL_NEAR_DOUBLET = 1,   /* another doublet entry (not the alpha = 0.5 mirror of the best one) within 1e-7 of the best */
       DMX_CELL_NEAR_SINGLET = 2,   /* the best two singlets within 1e-7 of each other, or a third within 1e-7 of the second */
       DMX_CELL_ORDER_CERTIFIED = 4, /* the order (j_best, k_best) of an alpha = 0.5 best doublet and llk12 are the reference's, bit for
                                       bit (device certificate, DESIGN.md "Ties"): the host tie arbiter has nothing left to decide */
       DMX_CELL_ORDER_RESOLVABLE = 8,/* the certificate stayed open over a single log() per accumulator: one host log() call each
                                       (dmx_write_doublet* do it) yields the reference's order and llk12 without the pileup */
       DMX_CELL_NEAR_RULE = 16      /* (ABI 7) one of the four comparisons of the BEST rule (cmd_cram_demuxlet.cpp:837,:844) — LLK12 > LLK1, LLK12 > LLK2,
                                       LLK12 > SNG.LLK1 + 2, SNG.LLK1 > SNG.LLK2 + 2 — has a margin below 1e-7: the device's log differs from libm's
                                       in the last bit of ~1.5 % of its evaluations, so SNG / DBL / AMB of such a barcode is decided by the writers from
                                       the (at most six) entries involved re-evaluated in the reference's operation order with the host libm */ };

int dmx_engine_create(const dmx_engine_config*, dmx_engine** out);
int dmx_engine_destroy(dmx_engine*);
/* Run every later launch/copy on this hipStream_t (e.g. torch's current stream). NULL = the engine's own stream. */
int dmx_engine_set_stream(dmx_engine*, void* hip_stream);
/* The phred LUT (host doubles from dmx_phred_tables, or the caller's own). Optional: defaults to dmx_phred_tables. */
int dmx_engine_set_phred_tables(dmx_engine*, const double mat[256], const double err[256]);
/* g[n_snps][n_samples][3] float32 (HOST or DEVICE memory). Also computes gp0s[n_snps][3] on the device (:390-401). */
int dmx_engine_set_genotypes(dmx_engine*, const float* g, int32_t n_snps, int32_t memory);
/* Stage the pileup: HOST arrays are copied to HBM; DEVICE arrays are adopted (caller keeps them alive). */
int dmx_engine_set_pileup(dmx_engine*, const dmx_pileup*);
/* K1: llks[B][V], llk0s[B] (:412-461).  Asynchronous on the engine's stream. */
int dmx_engine_run_singlet(dmx_engine*);
/* K2 (+K3): llksAB[B][V][V][A], llks00[B][A] (:576-710) and the per-cell summaries (:713-734,:746-758,:799-828). */
int dmx_engine_run_doublet(dmx_engine*);
/* Both in one call (ABI 5): K1 runs beside K2 on a low-priority stream of the engine and fills the slots K2's last round leaves free; fork
 * and join are events on the engine's stream (dmx_engine_set_stream), so the call orders like run_singlet + run_doublet.  Same bits. */
int dmx_engine_run(dmx_engine*);
int dmx_engine_sync(dmx_engine*);
/* Device->host copies of the results (any pointer may be NULL). Synchronises. */
int dmx_engine_get_singlet(dmx_engine*, double* llks, double* llk0s);
int dmx_engine_get_doublet(dmx_engine*, double* llksAB, double* llks00, dmx_cell_summary* summary);
/* sing[B][V] = llksAB[c][j][0][0], the singlet column of the grid (what .sing2 prints, :746-770) — lets a caller skip
 * the V*V*A grid entirely when --write-pair is off. */
int dmx_engine_get_sing(dmx_engine*, double* sing);
/* llksAB[V][V][A] of the n cells cells[0..n) (ids of the staged pileup) -> out[n][V][V][A]: the grids of the barcodes whose K3 record
 * carries a near-tie flag are all that a records-only consumer (dmx_write_doublet_summary, a multi-GPU gather) needs besides the records. */
int dmx_engine_get_cell_grids(dmx_engine*, const int32_t* cells, int32_t n, double* out);

/* (ABI 8) The `.pair` rows of `--write-pair` (cmd_cram_demuxlet.cpp:772-797, "%s\t%s\t%s\t%.3lf\t%.5lf\t%.5lg\n") formatted ON THE DEVICE from the grid that
 * already lies in HBM, packed in output order, ready for write(2) — instead of V + V(V-1)(A-1) rows per barcode through host threads.
 *   request   n_out barcodes in output order: `cells` = their ids in the staged pileup, `barcodes` / `sample_ids` the strings to print;
 *             host_rows[i] != 0: the caller prints this barcode's rows itself (the barcodes whose grid entries the tie arbiter may replace —
 *             dmx::cell_needs, a BEST-rule comparison within 1e-7 — dmx_demuxlet_run decides); ovr[i].n >= 0: the two certified entries of an
 *             alpha = 0.5 best doublet, llksAB[a][b][n] = llk_ab and llksAB[b][a][n] = llk_ba, to print instead of the device's own.
 *   text      LLK (`%.5lf`) is exact 128-bit integer arithmetic (printf's digits); POSTPRB (`%.5lg`) is printed only where its five digits cannot depend on the
 *             last bits of exp() — elsewhere (the denormal range, a value within 4e-13 of a rounding boundary) the field is left EMPTY and listed in
 *             `patches`: the caller inserts, at byte `offset` of the text, "%.5lg" of exp(value - maxLLK) * c / (sumSingle + sumDouble) computed with ITS
 *             libm (c = (1 - prior) / V for a singlet row, prior / V / (V-1) / (A-1) else; the record of barcode cells[out_cell] has the three scalars).
 *             cell_flag[i]: 0 = rows in the text at [cell_off[i], cell_off[i+1]); 1 = left to the caller as requested; 2 = left to the caller because
 *             an entry is not printable here (nan, inf, |v| >= 2^43), or because the barcode's maxLLK or sumSingle + sumDouble is not finite or the sum
 *             is not positive (a nan / inf in an entry that is never printed reaches them through the whole-grid scans) — both with an empty range:
 *             the caller's rows go in at cell_off[i].
 *   scalars   (appended, still ABI 8) The host formatter prints a barcode with certified entries from the grid WITH them: maxLLK and the two sums are
 *             those of that grid, not K3's record (up to 7e-12 STRICT / 6e-11 FAST apart — enough to move a fifth digit).  For a barcode with
 *             ovr[i].n >= 0 whose two values differ from the grid's bits the call reduces the three numbers again (K3's per-term expression over the
 *             grid with the two entries replaced); for every other barcode they are the record's.  dmx_pair_text_get_scalars returns them per OUTPUT
 *             barcode: they are what the text was printed from and what a patch must be computed from (not the record).
 *   limits    n_samples <= 4095, n_alpha <= 255 and 256 * (longest row) <= 150 KiB, where the longest row is taken as (longest barcode) + 2 * (longest
 *             sample id) + (longest "\t%.3lf\t" of an alpha) + 36 bytes; DMX_ERR_ARG otherwise.  dmx_demuxlet_run checks the same limits (over all
 *             barcodes of the job) and gives such a job to the host formatter.
 * Guaranteed, and tested as stated (tests/test_gpu_pair_text.py): the text with its patches filled in from the reported scalars, and the host's rows
 * at the flagged barcodes, is byte for byte what the host formatter prints from the grid with the certified entries substituted — also when a
 * certified entry moves a POSTPRB value across a rounding boundary, when a scalar is not finite, at any number of 256-row chunks, any output order
 * and any host_rows mask; a dmx_demuxlet_run `write_pair` job writes the same four files with the device formatter, with the host formatter
 * (DMX_PAIR_ON_HOST=1 behind DMX_EXPERIMENTS=1), and beyond the limits above. */
typedef struct { int32_t a, b, n, reserved; double llk_ab, llk_ba; } dmx_pair_override;   /* n < 0: none; else 0 <= a, b < n_samples, 0 <= n < n_alpha */
typedef struct { int64_t offset; double value; int32_t out_cell, singlet; } dmx_pair_patch;
typedef struct { double max_llk, sum_single, sum_double; } dmx_pair_scalars;
typedef struct {
  int32_t n_out;
  const int32_t* cells;             /* [n_out] */
  const char* const* barcodes;      /* [n_out] */
  const char* const* sample_ids;    /* [n_samples] */
  const uint8_t* host_rows;         /* [n_out] or NULL */
  const dmx_pair_override* ovr;     /* [n_out] or NULL */
} dmx_pair_request;
typedef struct dmx_pair_text dmx_pair_text;   /* owns the device text; host copies of the small arrays */
typedef struct {
  int64_t n_bytes; int32_t n_out, n_patches;
  const int64_t* cell_off;          /* [n_out + 1] */
  const uint8_t* cell_flag;         /* [n_out] */
  const dmx_pair_patch* patches;    /* [n_patches], ascending offset */
  double format_ms;                 /* HIP-event time of the three kernels */
} dmx_pair_text_info;
int  dmx_engine_format_pair(dmx_engine*, const dmx_pair_request*, dmx_pair_text** out);   /* needs run_doublet's results; synchronises */
int  dmx_pair_text_get_info(const dmx_pair_text*, dmx_pair_text_info* out);
int  dmx_pair_text_get_scalars(const dmx_pair_text*, const dmx_pair_scalars** out);      /* [n_out], owned by the text (a new entry point: the info struct is the caller's and cannot grow) */
int  dmx_pair_text_read(dmx_pair_text*, int64_t offset, int64_t n_bytes, void* dst);     /* device -> host copy of a piece of the text */
void dmx_pair_text_free(dmx_pair_text*);

/* Device views for zero-copy hand-off (torch tensors over them, RCCL gather of the per-cell records). */
typedef struct {
  double* llks;  double* llk0s;  double* llksAB;  double* llks00;  dmx_cell_summary* summary;  double* gp0s;
  double* sing;                /* [B][V] */
} dmx_device_view;
int dmx_engine_device_view(dmx_engine*, dmx_device_view* out);

/* HIP-event timing of the last launch of each kernel on the engine's stream, in milliseconds (0 when not run). */
typedef struct { float gp0_ms, singlet_ms, doublet_ms, reduce_ms; } dmx_kernel_times;
int dmx_engine_last_kernel_times(dmx_engine*, dmx_kernel_times* out);
/* The same, averaged over the launches since the last reset (at most the last 16 of each kernel): what a benchmark divides a
 * kernel's algorithmic bytes by.  doublet_ms is K2 alone, reduce_ms K3 alone, certify_ms K3b alone (0 when it does not run).
 * Synchronises the engine's stream.  reset != 0 forgets the launches seen so far; out may be NULL (reset only). */
typedef struct { double singlet_ms, doublet_ms, reduce_ms, certify_ms; int32_t n_singlet, n_doublet; } dmx_kernel_time_means;
int dmx_engine_mean_kernel_times(dmx_engine*, int32_t reset, dmx_kernel_time_means* out);
/* (ABI 7) Which kernels have run on the staged pileup, by the demangled names rocprofv3 prints ("k_doublet_a2<256, 4, 4, true, false, 32>";
 * empty = not run).  Each entry is what the LAST call that launches that kernel picked: run_singlet replaces `singlet`, run_doublet replaces
 * `doublet` and `certify` (empty when that run had no K3b), dmx_engine_run all three; staging a pileup clears them.  Where K1 ran: 0 = a launch of its own (run_singlet), 1 = beside K2 on the low-priority stream (dmx_engine_run), 2 = beside
 * K3 + K3b (dmx_engine_run when K2 leaves K1 no room).  A benchmark pairs its committed counter files with these names instead of guessing. */
typedef struct { char singlet[96], doublet[96], certify[96]; int32_t k1_placement; int32_t reserved[3]; } dmx_kernel_names;
int dmx_engine_kernel_names(dmx_engine*, dmx_kernel_names* out);
/* Algorithmic HBM bytes one launch of each kernel must move for the staged problem. */
typedef struct { double singlet_bytes, doublet_bytes, reduce_bytes; } dmx_kernel_bytes;
int dmx_engine_algorithmic_bytes(dmx_engine*, dmx_kernel_bytes* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Genotype refinement from called singlets (no counterpart in the reference).  For an assignment of barcodes to
 * samples (assign[b] = 0..V-1, or -1 = not used), over the staged pileup and phred tables, for every SNP i and sample v:
 *   LL[i][v][g]  = sum of log(GL_{b,i}[g]) over the barcodes b assigned to v that have a pair at SNP i — GL the reference's per-pair vector
 *                  after the +1e-6 renormalisation (cmd_cram_demuxlet.cpp:426-452); pairs whose stored reads are all allele 2 count too;
 *   n_cell[i][v] = the number of those pairs;  n_ref / n_alt[i][v] = their stored reads of allele 0 / 1;
 *   gp'[i][v][g] = q[g] exp(LL[g] - max LL) / sum over g of the same, q[g] = prior[i][v][g] + floor, in float64, rounded to float32;
 *                  a row with n_cell = 0 is prior's row, bit for bit (no floor).
 * Sum order: a sample's assigned barcodes in ascending cell id are cut into chunks of 64; inside a chunk the terms are added in barcode
 * order, then the chunk sums in ascending chunk order.  No floating-point atomics: the same inputs give the same bits, whatever ran before.
 * Operations (binary64, every product, sum and quotient rounded on its own; tests/contract_emul.cpp restates them and
 * tests/test_gpu_contract_bits.py compares the bits):
 *   GL        G = (1, 1, 1); per stored read in stored order, with mat / err the phred tables at its base quality, e3 = err / 3 and
 *             h = 0.5 - err / 3 (each rounded once):  G_0 *= allele 1 ? e3 : mat,  G_1 *= h,  G_2 *= allele 1 ? mat : e3,
 *             t = (G_0 + G_1) + G_2,  G_g = G_g / t (IEEE division);  after the last read G_g += 1e-6, t = (G_0 + G_1) + G_2, G_g = G_g / t.
 *             A pair without stored reads is the last step alone on (1, 1, 1).  (The kernels start from tables of these values and divide
 *             by a refined reciprocal where that is correctly rounded: the same bits.)
 *   log       dmx_log; its arguments are >= 1e-6 / (1 + 3e-6), never outside the positive normal numbers.
 *   sums      a chunk's sum starts at +0 and takes the logs of its barcodes' pairs at the SNP in barcode order; LL starts at +0 and takes the
 *             chunk sums in chunk order (a chunk without a pair at the SNP adds +0).
 * The call runs on the engine's stream and synchronises it before returning (the prior may be freed then).  It leaves every other result
 * of the engine as it was. */
typedef struct {
  int32_t n_cells;             /* = the staged pileup's n_cells */
  int32_t assign_memory;       /* DMX_MEM_HOST or DMX_MEM_DEVICE: where `assign` lives */
  const int32_t* assign;       /* [n_cells] */
  int32_t n_snps;              /* = the genotype matrix's n_snps */
  int32_t reserved0;
  const float* prior;          /* [n_snps][V][3] float32, HOST (normally the matrix the engine was given) */
  double  floor;               /* >= 0; 1e-3 is the usual value */
  int32_t reserved[4];         /* 0 */
} dmx_refine_request;
typedef struct {
  double  blocks_ms;           /* HIP-event times: the slab table (k_snp_blocks; 0 when the staged pileup's table already existed), */
  double  partial_ms;          /* k_refine_partial + k_refine_fold over all waves, */
  double  finish_ms;           /* k_refine_finish */
  int64_t partial_bytes;       /* device bytes of one wave of chunk partials */
  int32_t n_chunks, n_waves, chunk_cells, slab_snps, n_assigned;
  int32_t reserved[3];
} dmx_refine_info;
int dmx_engine_refine_genotypes(dmx_engine*, const dmx_refine_request*);
/* Device->host copies of the last refinement (any pointer may be NULL): llk[S][V][3] f64, n_cell / n_ref / n_alt [S][V] i32, gp[S][V][3] f32. */
int dmx_engine_get_refined(dmx_engine*, double* llk, int32_t* n_cell, int32_t* n_ref, int32_t* n_alt, float* gp);
/* The device pointer of the last gp' (for dmx_engine_set_genotypes(..., DMX_MEM_DEVICE) without a round trip).  Valid until the engine is
 * destroyed; a later refinement writes its gp' to the OTHER of two buffers when this one is the engine's genotype matrix, else may reuse it. */
int dmx_engine_refined_device_ptr(dmx_engine*, const float** out);
int dmx_engine_refine_info(dmx_engine*, dmx_refine_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Genotype-free clustering (no counterpart in the reference): the pieces of an EM over C = V columns of cluster
 * genotypes, driven by demuxlet_amd/cluster.py.  The E-step's likelihoods are K1's llks (dmx_engine_run_singlet with the columns as the
 * genotype matrix); these calls add the rest.  Each runs on the engine's stream, synchronises it before returning (host inputs may be
 * freed then) and leaves every other result of the engine as it was.
 *
 * dmx_engine_cluster_stage: a cache of the staged pileup in SNP-major order, ascending cell id inside a SNP — per pair (slot j) the cell
 *   id, lgl[j][g] = log GL[g] (the refinement's per-pair vector, section 12, and its log) and the stored REF / ALT reads; snp_off[S + 1]
 *   gives each SNP's slots.  Dense layouts place pair t of cell b at slot t * B + b; sparse ones at snp_off[s] + the number of
 *   barcodes of lower id with a pair at s, counted per group of barcodes and SNP slab in LDS (a stable counting sort keyed by SNP; no
 *   atomics decide a slot).  About 32 bytes per pair: DMX_ERR_NOMEM, and no cache, when that and the placement's scratch do not fit
 *   the free device memory; DMX_ERR_ARG for a sparse pileup of 2^31 pairs or more, or a pair of more than 65 535 stored reads.  The cache is a snapshot: staging a pileup again leaves it alone (the E-step and the M-step check that
 *   the barcode and SNP counts agree); the next dmx_engine_cluster_stage replaces it.
 *
 * dmx_engine_cluster_mstep: for weights w[B][C] (float64) and a per-SNP prior q[S][3] (float32, host), for every SNP i and column c:
 *   LL[i][c][g] = sum over the slots of SNP i of w[b][c] * lgl[g],  W[i][c] = sum of w[b][c],
 *   gp'[i][c][g] = (q[i][g] + floor) exp(LL[g] - max LL) / sum over g of the same, in float64, rounded to float32; a row with W = 0 is
 *   q's row, bit for bit.  Sum order: the slots of a SNP in ascending cell id, one after the other, as acc = fma(w, lgl, acc) from 0
 *   (W: acc += w); no floating-point atomics, so the bits depend neither on the launch geometry nor on what ran before.  gp' goes to
 *   the OTHER of two buffers when the current one is the engine's genotype matrix (dmx_engine_set_genotypes(..., DMX_MEM_DEVICE) with
 *   dmx_engine_cluster_device_ptr), so an M-step never overwrites the matrix K1 reads.  lgl[j][g] is dmx_log of the refinement's G_g,
 *   operation for operation (section 12's block above); fma is the correctly rounded fused multiply-add, its first operand the weight
 *   w[b][c] read as stored (0, 1 and 1e-300 are weights like any other); LL and W of a SNP without slots are +0
 *   (tests/contract_emul.cpp, tests/test_gpu_contract_bits.py).
 *
 * dmx_engine_cluster_estep: from K1's llks[B][C] of the last run_singlet, C = R * K columns grouped as R restarts x K clusters, per
 *   barcode b and restart r:  a_k = (llks[b][rK + k] + log_pi[r][k]) / T,  w[b][rK + k] = exp(a_k - max a) / sum over k;  a barcode
 *   with mask[b] = 0 gets w = 0.  ll[r] = sum over the barcodes in the mask of logsumexp_k(llks[b][rK + k] + log_pi[r][k]), col_sum[c]
 *   = sum over b of w[b][c].  Both sums add the barcodes in chunks of 256 in barcode order, then the chunk sums in ascending order
 *   (no atomics).  The weights stay on the device for the next M-step (DMX_CLUSTER_LAST_ESTEP). */
enum { DMX_CLUSTER_LAST_ESTEP = 2 };   /* dmx_cluster_mstep_request.weights_memory: the weights of the last dmx_engine_cluster_estep */
typedef struct {
  int32_t n_cells;             /* = the cache's barcodes */
  int32_t n_snps;              /* = the cache's SNPs = the genotype matrix's n_snps */
  int32_t n_cols;              /* C = the engine's V */
  int32_t weights_memory;      /* DMX_MEM_HOST, DMX_MEM_DEVICE or DMX_CLUSTER_LAST_ESTEP (weights ignored) */
  const double* weights;       /* [n_cells][n_cols] float64 */
  const float* prior;          /* [n_snps][3] float32, HOST */
  double  floor;               /* >= 0; 1e-3 is the usual value */
  int32_t reserved[4];         /* 0 */
} dmx_cluster_mstep_request;
typedef struct {
  int32_t n_restarts, n_clusters;   /* R, K: R * K = the engine's V */
  const double* log_pi;        /* [R][K] HOST */
  double  temperature;         /* T > 0; 1 is plain EM */
  const uint8_t* mask;         /* [B] HOST, or NULL = every barcode */
  double* ll;                  /* [R] HOST out (may be NULL) */
  double* col_sum;             /* [R * K] HOST out (may be NULL) */
  int32_t reserved[4];         /* 0 */
} dmx_cluster_estep_request;
typedef struct {
  double  stage_ms;            /* HIP-event times of the last stage (sort + k_cluster_lgl), */
  double  mstep_ms;            /* ... of the last M-step (k_cluster_mstep), */
  double  estep_ms;            /* ... and of the last E-step (k_cluster_estep + the ordered sums) */
  int64_t cache_bytes;         /* device bytes of the stage cache */
  int64_t scratch_bytes;       /* device bytes the stage borrowed while it ran (sparse layouts: the placement) */
  int64_t n_pairs;             /* slots of the cache */
  int32_t n_cells, n_snps, sorted, n_cols;   /* sorted: 1 = a sparse layout went through the placement; n_cols: the last M-step's */
  int32_t reserved[2];
} dmx_cluster_info;
int dmx_engine_cluster_stage(dmx_engine*);
int dmx_engine_cluster_mstep(dmx_engine*, const dmx_cluster_mstep_request*);
int dmx_engine_cluster_estep(dmx_engine*, const dmx_cluster_estep_request*);
/* Device->host copies of the last M-step (any pointer may be NULL): ll[S][C][3] f64, wsum[S][C] f64, gp[S][C][3] f32; and of the last
 * E-step's weights[B][C] f64 (DMX_ERR_STATE when that part has not run). */
int dmx_engine_get_cluster(dmx_engine*, double* ll, double* wsum, float* gp, double* weights);
/* Device->host copy of the stage cache (any pointer may be NULL): snp_off[S + 1] i64, cell[P] i32, lgl[P][3] f64, ref_alt[P] u32
 * (REF reads | ALT reads << 16). */
int dmx_engine_get_cluster_stage(dmx_engine*, int64_t* snp_off, int32_t* cell, double* lgl, uint32_t* ref_alt);
/* The device pointer of the last M-step's gp' [S][C][3] (for dmx_engine_set_genotypes(..., DMX_MEM_DEVICE)); valid until the engine is
 * destroyed. */
int dmx_engine_cluster_device_ptr(dmx_engine*, const float** out);
int dmx_engine_cluster_info(dmx_engine*, dmx_cluster_info* out);

/* Doublet-aware clustering (no counterpart in the reference): doublets of two clusters of the same restart as
 * components of the EM, so that their reads do not pull any cluster's genotypes toward heterozygous.
 *
 * dmx_engine_cluster_doublet: with the engine's V = R * K columns read as R restarts x K clusters, for every barcode b, restart r and
 *   pair p = (k, l), k < l, numbered lexicographically (P = K (K - 1) / 2 pairs), over the staged pileup, the phred tables and the
 *   genotype matrix gp (float32) that K1 reads:
 *     LLD[b][r][p] = sum over b's pairs in ascending SNP order of log(sum over x, y of gp[i][rK + k][x] gp[i][rK + l][y] pG[x + y]),
 *   pG[s] the reference's per-pair doublet factors at alpha = 0.5 (cmd_cram_demuxlet.cpp:594-663; weight s / 4, five distinct values):
 *   per stored read the products, then division by their maximum; then + 1e-6 and the same renormalisation.  With the alpha grid
 *   {0, 0.5} that maximum is the reference's, so LLD = the reference's llksAB[b][rK + k][rK + l][alpha = 0.5] up to rounding; the log
 *   is dmx_log.  Each (b, r, p) is one serial sum with no floating-point atomics: the bits do not depend on R, on the position of
 *   the restart's columns in the engine, or on what ran before.  Beside it, per barcode, lsc[b] = the sum over its pairs in the same
 *   order of log(pG[0] + pG[2] + pG[4]): pG[2x] is the singlet genotype x's factor on the doublet's max-normalised scale, so
 *   LLD - lsc is on the sum-normalised scale of K1's llks (the E-step compares the two).  DMX_ERR_ARG: K < 2 or R * K != V;
 *   DMX_ERR_NOMEM: the B x (R x P + 1) float64 result does not fit the free device memory; DMX_ERR_STATE: no pileup or no genotypes.
 *   Staging a pileup again drops it.
 *
 * dmx_engine_cluster_estep_doublet: the E-step over K singlet and P doublet components per (barcode, restart), from K1's llks of the
 *   last run_singlet and the LLD of the last dmx_engine_cluster_doublet (same R and K).  Log priors: singlet k log(1 - delta_r) +
 *   log pi_rk; doublet (k, l) log delta_r + log(2 pi_rk pi_rl / (1 - sum over k of pi_rk^2)).  The singlet llk is K1's llks[b][rK + k],
 *   the doublet llk LLD[b][r][p] - lsc[b].  Every score is (llk + log prior) / T;
 *   w[b][rK + k] = the singlet components' posteriors (they sum to 1 - m_b,r, m_b,r the doublet components' total),
 *   ll[r] = sum over the barcodes in the mask of logsumexp over all K + P components of llk + log prior, col_sum[c] = sum over b of
 *   w[b][c], dbl_mass[r] = sum over b of m_b,r; the sums are those of dmx_engine_cluster_estep (chunks of 256 barcodes, then the chunks
 *   in order).  log_delta[r] = -inf (delta = 0) gives dmx_engine_cluster_estep's results.  The weights stay on the device for the next
 *   M-step (DMX_CLUSTER_LAST_ESTEP) and dmx_engine_get_cluster returns them.  DMX_ERR_ARG: a log_delta that is NaN or >= 0. */
typedef struct {
  int32_t n_restarts, n_clusters;   /* R, K: R * K = the engine's V, K >= 2 */
  const double* log_pi;        /* [R][K] HOST */
  const double* log_delta;     /* [R] HOST: log of each restart's doublet share, < 0; -inf = no doublets */
  double  temperature;         /* T > 0; 1 is plain EM */
  const uint8_t* mask;         /* [B] HOST, or NULL = every barcode */
  double* ll;                  /* [R] HOST out (may be NULL) */
  double* col_sum;             /* [R * K] HOST out (may be NULL) */
  double* dbl_mass;            /* [R] HOST out (may be NULL) */
  int32_t reserved[4];         /* 0 */
} dmx_cluster_estep_doublet_request;
typedef struct {
  double  doublet_ms;          /* HIP-event time of the last dmx_engine_cluster_doublet (k_cluster_dbl) */
  double  estep_ms;            /* ... and of the last doublet E-step (k_cluster_estep_dbl + the ordered sums) */
  int64_t lld_bytes;           /* device bytes of LLD[B][R][P] and lsc[B] */
  int32_t n_cells, n_restarts, n_clusters, n_pairs;   /* n_pairs: P = K (K - 1) / 2 per restart */
  int32_t reserved[4];
} dmx_cluster_doublet_info;
int dmx_engine_cluster_doublet(dmx_engine*, int32_t n_restarts, int32_t n_clusters);
/* Device->host copies of the last LLD (either pointer may be NULL): lld[B][R][P] f64, lsc[B] f64 (DMX_ERR_STATE before a run). */
int dmx_engine_get_cluster_doublet(dmx_engine*, double* lld, double* lsc);
int dmx_engine_cluster_estep_doublet(dmx_engine*, const dmx_cluster_estep_doublet_request*);
int dmx_engine_cluster_doublet_info(dmx_engine*, dmx_cluster_doublet_info* out);

/* Split-merge moves for the clustering EM (no counterpart in the reference), driven by demuxlet_amd/cluster.py.
 *
 * dmx_engine_cluster_merge_score: for the last M-step's C = R * K columns read as R restarts x K clusters, with the M-step's own genotype
 *   prior log pi[i][g] = log((prior[i][g] + floor) / sum over g of (prior[i][g] + floor)) (prior [S][3] float32, HOST) and its LL[i][c][g]
 *   and W[i][c], for every restart r and pair p = (k, l), k < l, numbered lexicographically (P = K (K - 1) / 2):
 *     bf[r][p] = sum over the SNPs i with W[i][rK + k] > 0 and W[i][rK + l] > 0 of
 *                (lse_g(log pi[i][g] + LL[i][rK + k][g] + LL[i][rK + l][g]) - A[i][rK + k]) - A[i][rK + l],
 *     A[i][c] = lse_g(log pi[i][g] + LL[i][c][g]),  n_shared[r][p] = the number of those SNPs;
 *   the log Bayes factor "one donor" against "two donors" of the two clusters' pooled genotype likelihoods.  Other SNPs add exactly 0.
 *   Sum order: the SNPs in chunks of 256 in ascending order, each chunk serially from 0, then the chunks in ascending order; no
 *   floating-point atomics, so the bits depend neither on the launch geometry, R, the position of the restart's columns nor on what
 *   ran before.  bf [R][P] f64 and n_shared [R][P] i32 are HOST outputs (either may be NULL).  DMX_ERR_STATE: no M-step on the stage
 *   cache; DMX_ERR_ARG: R * K != the last M-step's columns, K outside [2, 64], a missing prior or a bad floor.
 *
 * dmx_engine_cluster_estep_grouped: dmx_engine_cluster_estep's arithmetic, except that restart r sees only the barcodes b with
 *   group[b] == r / restarts_per_group (and in the mask): every other barcode gets w = 0 and adds nothing to ll[r] or col_sum.  The
 *   sums are those of dmx_engine_cluster_estep.  With one group holding every barcode and restarts_per_group = R the results are
 *   dmx_engine_cluster_estep's, bit for bit.  The weights stay on the device for the next M-step (DMX_CLUSTER_LAST_ESTEP).
 *   DMX_ERR_ARG: R * K != V, a restarts_per_group that does not divide R, a missing group or a group id outside [-1, R / restarts_per_group). */
typedef struct {
  int32_t n_restarts, n_clusters;   /* R, K: R * K = the engine's V */
  const double* log_pi;        /* [R][K] HOST */
  double  temperature;         /* T > 0; 1 is plain EM */
  const uint8_t* mask;         /* [B] HOST, or NULL = every barcode */
  const int32_t* group;        /* [B] HOST: the group of each barcode, -1 = none */
  int32_t restarts_per_group;  /* restarts r .. r + restarts_per_group - 1 of group r / restarts_per_group */
  int32_t reserved0;           /* 0 */
  double* ll;                  /* [R] HOST out (may be NULL) */
  double* col_sum;             /* [R * K] HOST out (may be NULL) */
  int32_t reserved[4];         /* 0 */
} dmx_cluster_estep_grouped_request;
typedef struct {
  double  merge_ms;            /* HIP-event time of the last merge score (k_cluster_marg + k_cluster_merge_part + k_cluster_merge_fold) */
  double  grouped_estep_ms;    /* ... and of the last grouped E-step (k_cluster_estep_grp + the ordered sums) */
  int32_t n_restarts, n_clusters, n_pairs, n_chunks;   /* of the last merge score */
  int32_t reserved[4];
} dmx_cluster_sm_info;
int dmx_engine_cluster_merge_score(dmx_engine*, int32_t n_restarts, int32_t n_clusters, const float* prior, double floor, double* bf, int32_t* n_shared);
int dmx_engine_cluster_estep_grouped(dmx_engine*, const dmx_cluster_estep_grouped_request*);
int dmx_engine_cluster_sm_info(dmx_engine*, dmx_cluster_sm_info* out);

/* Choosing the number of clusters (no counterpart in the reference), driven by demuxlet_amd/cluster.py: a merge
 * path from an over-specified K downwards, every state scored by the model evidence of its hard labels.  A column that has been merged
 * away is "inactive": the driver gives it log_pi = -inf in the E-steps above, which then give it weights of exactly 0.
 *
 * dmx_engine_cluster_evidence: for the last M-step's C = R * K columns, with dmx_engine_cluster_merge_score's genotype prior log pi[i][g],
 *     ev[r][k] = sum over the SNPs i with W[i][rK + k] > 0 of A[i][rK + k],  A[i][c] = lse_g(log pi[i][g] + LL[i][c][g]),
 *   the log marginal likelihood of the column's reads with the genotypes integrated out, and n_cov[r][k] = the number of those SNPs.
 *   A SNP with W = 0 adds nothing, so an empty column has ev = 0.0 and n_cov = 0.  Sum order: the merge score's (the SNPs in chunks of
 *   256 in ascending order, each chunk serially from 0, then the chunks in ascending order; no floating-point atomics), so the bits
 *   depend neither on the launch geometry, R, the position of the restart's columns nor on what ran before, and for a pair (k, l) the
 *   evidence of the merged column minus ev[k] and ev[l] is bf[(k, l)] up to rounding.  ev [R * K] f64 and n_cov [R * K] i32 are HOST
 *   outputs (either may be NULL).  DMX_ERR_STATE: no M-step on the stage cache; DMX_ERR_ARG: R * K != the last M-step's columns, K
 *   outside [1, 64], a missing prior or a bad floor.
 *
 * dmx_engine_cluster_hard: hard labels from the weights w[B][R * K] of the last E-step of any kind.  Per barcode b and restart r:
 *     mask[b] = 0:                                    label = -1;
 *     doublets and the doublet mass m_b,r >= 0.5:     label = -2 - p, p the pair (k, l) of two active columns with the highest
 *                                                     LLD[b][r][p] (the lowest p on a tie), which is the barcode's doublet score;
 *     otherwise:                                      label = the active k with the highest w[b][rK + k] (the lowest k on a tie).
 *   With doublets = 1 the doublet mass is that of the last dmx_engine_cluster_estep_doublet, which must be the last E-step, and LLD that
 *   of the last dmx_engine_cluster_doublet (same R and K).  n_sing[r][k] counts the barcodes labelled k, n_dbl[r] the doublet-labelled
 *   ones, dbl_score[r] is the sum of their doublet scores in dmx_engine_cluster_estep's order (chunks of 256 barcodes in barcode order,
 *   then the chunks in ascending order; other barcodes add nothing).  It is on LLD's scale: minus the sum of lsc[b] over those barcodes it
 *   is on K1's and the evidence's (dmx_engine_cluster_doublet).  On the device the call leaves a one-hot matrix [B][R * K] f64,
 *   1.0 at a singlet-labelled barcode's column and 0.0 elsewhere, in a buffer of its own (dmx_engine_cluster_hard_device_ptr; the
 *   M-step takes it as DMX_MEM_DEVICE): the E-step's weights are only read.  DMX_ERR_STATE: no E-step weights, or doublets = 1 without
 *   that doublet mass or those doublet likelihoods; DMX_ERR_ARG: R * K != the weights' columns, a missing `active`, a restart with no
 *   active column, or doublets = 1 with fewer than two active columns in a restart.
 *
 * dmx_engine_cluster_merge_columns: edits the last E-step's weights in place.  For every barcode and every restart r with from[r] >= 0:
 *   w[into[r]] = w[into[r]] + w[from[r]] (one addition), then w[from[r]] = 0.0; a restart with from[r] = -1 is untouched.  The next
 *   M-step takes the result as DMX_CLUSTER_LAST_ESTEP.  from / into are [R] HOST.  DMX_ERR_STATE: no E-step weights; DMX_ERR_ARG:
 *   R * K != the weights' columns, from == into, or an index outside [0, K) (from: [-1, K)). */
typedef struct {
  int32_t n_restarts, n_clusters;   /* R, K: R * K = the columns of the last E-step's weights */
  int32_t doublets;            /* 1: doublet labels from the last doublet E-step's mass and the last LLD */
  int32_t reserved0;           /* 0 */
  const uint8_t* active;       /* [R * K] HOST: 1 = the column takes part */
  const uint8_t* mask;         /* [B] HOST, or NULL = every barcode */
  int32_t* label;              /* [B][R] HOST out (may be NULL) */
  int32_t* n_sing;             /* [R * K] HOST out (may be NULL) */
  int32_t* n_dbl;              /* [R] HOST out (may be NULL) */
  double* dbl_score;           /* [R] HOST out (may be NULL) */
  int32_t reserved[4];         /* 0 */
} dmx_cluster_hard_request;
typedef struct {
  double  evidence_ms;         /* HIP-event times of the last evidence (k_cluster_marg + k_cluster_ev_part + k_cluster_ev_fold), */
  double  hard_ms;             /* ... of the last hard labels (k_cluster_hard + k_cluster_hard_part + k_cluster_hard_fold), */
  double  merge_columns_ms;    /* ... and of the last column merge (k_cluster_merge_cols) */
  int32_t n_restarts, n_clusters, n_chunks, n_cells;   /* R, K and the SNP chunks of the last evidence; the barcodes of the last hard labels */
  int32_t reserved[4];
} dmx_cluster_k_info;
int dmx_engine_cluster_evidence(dmx_engine*, int32_t n_restarts, int32_t n_clusters, const float* prior, double floor, double* ev, int32_t* n_cov);
int dmx_engine_cluster_hard(dmx_engine*, const dmx_cluster_hard_request*);
/* The device pointer of the last one-hot matrix [B][R * K] f64 (DMX_ERR_STATE before dmx_engine_cluster_hard); valid until the next
 * dmx_engine_cluster_hard or dmx_engine_cluster_stage. */
int dmx_engine_cluster_hard_device_ptr(dmx_engine*, const double** out);
/* Device->host copies of the last hard labels (any pointer may be NULL): label[B][R] i32, score[B][R] f64 (each barcode's doublet
 * score, 0.0 unless doublet-labelled), hot[B][R * K] f64 (the one-hot matrix), and dbl_mass[B][R] f64, the doublet mass the labels
 * were made from (DMX_ERR_STATE when they were made with doublets = 0, or before dmx_engine_cluster_hard). */
int dmx_engine_get_cluster_hard(dmx_engine*, int32_t* label, double* score, double* hot, double* dbl_mass);
int dmx_engine_cluster_merge_columns(dmx_engine*, int32_t n_restarts, int32_t n_clusters, const int32_t* from, const int32_t* into);
int dmx_engine_cluster_k_info(dmx_engine*, dmx_cluster_k_info* out);

/* Partly genotyped pools (no counterpart in the reference), driven by demuxlet_amd/partial.py: Vk donors are
 * known from the VCF and M more are learned by the clustering EM in R restarts.  The engine's V = Vk + R * M columns are
 * [the Vk known donors | restart 0's M free columns | ... | restart R-1's M], so K1 scores the known columns once for all restarts.
 *
 * dmx_engine_cluster_set_known: the known rows g[n_snps][n_known][3] (float32, DMX_MEM_HOST or DMX_MEM_DEVICE); the engine keeps a
 *   device copy.  n_known = 0 is accepted.  DMX_ERR_ARG: n_known outside [0, V), a missing pointer or a bad memory kind.
 *
 * dmx_engine_cluster_estep_known: from K1's llks[B][V] of the last run_singlet, per barcode b and restart r over its Vk + M components
 *   (component k < Vk: column k; component Vk + m: column Vk + r M + m):  a_k = (llks[b][col] + log_pi[r][k]) / T,
 *   w_k = exp(a_k - max a) / sum over k;  a barcode with mask[b] = 0 gets w = 0 and is left out of ll.  ll[r] = sum over the barcodes in
 *   the mask of logsumexp_k(llks + log_pi), col_sum[r][k] = sum over b of w_k; the sums are those of dmx_engine_cluster_estep (chunks
 *   of 256 barcodes in order, then the chunks in order; no atomics).  The free weights w[B][R * M] stay on the device for the next
 *   windowed M-step (DMX_CLUSTER_LAST_ESTEP) and dmx_engine_get_cluster returns them; dmx_engine_get_cluster_known returns all
 *   components' weights [B][R][Vk + M].  With n_known = 0 every result is dmx_engine_cluster_estep's (R, K = M), bit for bit.
 *   DMX_ERR_ARG: Vk + R * M != V, M < 1, Vk < 0, a missing log_pi or a bad temperature.
 *
 * dmx_engine_cluster_mstep_window: dmx_engine_cluster_mstep's arithmetic and sum order over the R * M free columns only, weights
 *   w[B][R * M]: LL[S][R * M][3] and W[S][R * M] (dmx_engine_get_cluster, dmx_engine_cluster_merge_score), and gp' into columns
 *   Vk .. V-1 of a [S][V][3] buffer whose columns 0 .. Vk-1 hold the known rows of dmx_engine_cluster_set_known, bit for bit.  The
 *   buffer is double-buffered as dmx_engine_cluster_mstep's (dmx_engine_cluster_device_ptr).  With no known columns every result is
 *   dmx_engine_cluster_mstep's, bit for bit.  DMX_ERR_STATE: no stage cache or no known rows; DMX_ERR_ARG: Vk + R * M != V, M < 1, or
 *   counts that disagree with the stage cache or the known rows. */
typedef struct {
  int32_t n_restarts, n_known, n_free;   /* R, Vk, M: Vk + R * M = the engine's V; Vk >= 0, M >= 1 */
  int32_t reserved0;           /* 0 */
  const double* log_pi;        /* [R][Vk + M] HOST */
  double  temperature;         /* T > 0; 1 is plain EM */
  const uint8_t* mask;         /* [B] HOST, or NULL = every barcode */
  double* ll;                  /* [R] HOST out (may be NULL) */
  double* col_sum;             /* [R][Vk + M] HOST out (may be NULL) */
  int32_t reserved[4];         /* 0 */
} dmx_cluster_estep_known_request;
typedef struct {
  int32_t n_cells;             /* = the cache's barcodes */
  int32_t n_snps;              /* = the cache's SNPs = the known rows' */
  int32_t n_restarts, n_free;  /* R, M: the known rows' Vk + R * M = the engine's V */
  int32_t weights_memory;      /* DMX_MEM_HOST, DMX_MEM_DEVICE or DMX_CLUSTER_LAST_ESTEP (weights ignored) */
  int32_t reserved0;           /* 0 */
  const double* weights;       /* [n_cells][R * M] float64 */
  const float* prior;          /* [n_snps][3] float32, HOST */
  double  floor;               /* >= 0; 1e-3 is the usual value */
  int32_t reserved[4];         /* 0 */
} dmx_cluster_mstep_window_request;
typedef struct {
  double  estep_ms;            /* HIP-event times of the last known-column E-step (k_cluster_estep_known + the ordered sums) */
  double  mstep_ms;            /* ... and of the last windowed M-step (the known rows' copy + k_cluster_mstep_win) */
  int32_t n_cells, n_known, n_restarts, n_free;
  int32_t reserved[4];
} dmx_cluster_known_info;
int dmx_engine_cluster_set_known(dmx_engine*, int32_t n_snps, int32_t n_known, const float* g, int32_t memory);
int dmx_engine_cluster_estep_known(dmx_engine*, const dmx_cluster_estep_known_request*);
int dmx_engine_cluster_mstep_window(dmx_engine*, const dmx_cluster_mstep_window_request*);
/* Device->host copy of the last known-column E-step's weights [B][R][Vk + M] f64 (DMX_ERR_STATE before one). */
int dmx_engine_get_cluster_known(dmx_engine*, double* weights);
int dmx_engine_cluster_known_info(dmx_engine*, dmx_cluster_known_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Ambient contamination profile (no counterpart in the reference).  Soup is the average of many lysed cells: at
 * SNP i its reads are ALT with a fixed frequency a_i.  For an assignment of barcodes to samples (assign[b] = 0..V-1, or -1 = not used),
 * ambient ALT frequencies a[n_snps] and a grid of contamination fractions rho[q], q < Q, over the staged pileup, the phred tables and
 * the engine's genotype matrix gp (float32), for every assigned barcode b (v = assign[b]) and every q:
 *   p_g(rho) = (1 - rho) g / 2 + rho a_i  (g = 0, 1, 2);
 *   f_g      = product over the pair's stored reads, in stored order, of pR (1 - p_g) + pA p_g, pR = allele 0 ? mat[bq] : err[bq] / 3,
 *              pA = allele 1 ? mat[bq] : err[bq] / 3 (the reference's per-read doublet factor, cmd_cram_demuxlet.cpp:606-625, with the
 *              second genotype replaced by the soup);
 *   LL[b][q] = sum over b's pairs in ascending SNP order of log(gp[i][v][0] f_0 + gp[i][v][1] f_1 + gp[i][v][2] f_2).
 * No per-read renormalisation and no 1e-6 floor: at rho = 0 this is the likelihood of the reads under the called genotype.  A pair with
 * no stored read, or whose gp row is all zero, contributes nothing; n_snp[b] / n_read[b] count the pairs / reads that did.  f_g is kept
 * in range by exact power-of-two rescaling, the exponent carried into the log; the log is dmx_log.  Each (b, q) is one serial sum with
 * no floating-point atomics: the same inputs give the same bits whatever the grid's length or what ran before, and a grid split over
 * two calls gives the same bits at the shared points.  Unassigned barcodes get zero rows.
 * Operations (binary64, every product and sum rounded on its own: no contraction; tests/contract_emul.cpp restates them and
 * tests/test_gpu_contract_bits.py compares the bits):
 *   p_g       om = 1 - rho,  ra = rho a_i;  p_0 = ra,  p_1 = 0.5 om + ra,  p_2 = om + ra;  q_g = 1 - p_g, rounded once;
 *   factor    e3 = err[bq] / 3 rounded once;  t_g = pR q_g + pA p_g (two products, one sum);  f_g = t_g of the first stored read, then
 *             f_g = f_g t_g read by read;
 *   rescale   only in a pair of 8 or more stored reads.  After the first read's factor, f_g of an entry with gp[i][v][g] = 0 is set to 0,
 *             so that the scale follows the entries that count.  After every eighth read (the pair's reads 8, 16, ...), with
 *             mx = max(f_0, f_1, f_2): when 0 < mx < 2^-300, e = the exponent of mx as frexp gives it (mx = m 2^e, 0.5 <= m < 1), every
 *             f_g = ldexp(f_g, -e) and E += e (E starts at 0 for every pair);
 *   term      L = (gp_0 f_0 + gp_1 f_1) + gp_2 f_2 with the float32 entries widened;  lg = dmx_log(L), and when E != 0
 *             lg = fma(E, DMX_LOG_LN2HI, fma(E, DMX_LOG_LN2LO, lg)), the two parts of ln 2 of csrc/dmx_log.hpp;
 *   sum       LL[b][q] starts at +0 and takes lg pair by pair.
 * An L that is not a positive normal number goes to the runtime's log instead of dmx_log; on these paths that is L = 0 only (every
 * counted product is 0, which takes phred tables with a zero entry), and the term and LL[b][q] are -inf.
 * The call runs on the engine's stream,
 * synchronises it before returning (host inputs may be freed then) and leaves every other result of the engine as it was.
 * DMX_ERR_ARG: Q outside [1, 256], a grid point outside [0, 1] or not strictly ascending, an a_i outside [0, 1], assign[b] outside
 * [-1, V), n_cells / n_snps that do not match the staged pileup / the genotype matrix.  DMX_ERR_STATE: no pileup or no genotypes yet.
 * DMX_ERR_NOMEM: the B x Q profile does not fit the free device memory. */
typedef struct {
  int32_t n_cells;             /* = the staged pileup's n_cells */
  int32_t assign_memory;       /* DMX_MEM_HOST or DMX_MEM_DEVICE: where `assign` lives */
  const int32_t* assign;       /* [n_cells] */
  int32_t n_snps;              /* = the genotype matrix's n_snps */
  int32_t n_grid;              /* Q, 1..256 */
  const double* ambient;       /* [n_snps] float64 in [0, 1], HOST */
  const double* grid;          /* [n_grid] float64, strictly ascending, in [0, 1], HOST */
  int32_t reserved[4];         /* 0 */
} dmx_ambient_request;
typedef struct {
  double  kernel_ms;           /* HIP-event time of the last call's k_ambient */
  int64_t profile_bytes;       /* device bytes of the B x Q profile */
  int32_t n_cells, n_grid, n_assigned;
  int32_t reserved[3];
} dmx_ambient_info;
int dmx_engine_ambient(dmx_engine*, const dmx_ambient_request*);
/* Device->host copies of the last profile (any pointer may be NULL): ll[B][Q] f64, n_snp[B] / n_read[B] i32. */
int dmx_engine_get_ambient(dmx_engine*, double* ll, int32_t* n_snp, int32_t* n_read);
int dmx_engine_ambient_info(dmx_engine*, dmx_ambient_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Ambient-aware doublet profile (no counterpart in the reference): the doublet likelihood with the soup term of
 * dmx_engine_ambient, so that a soupy singlet and a doublet can be compared on one scale.  For up to C candidate sample pairs per
 * barcode, cand[b][c] = (v1, v2) with v1 = -1 = slot not used and otherwise 0 <= v1, v2 < V, v1 != v2, mixing shares alpha[n], n < A
 * (the share of v2's reads), ambient ALT frequencies a[n_snps] and contamination fractions rho[q], q < Q, over the staged pileup, the
 * phred tables and the engine's genotype matrix gp (float32), for every barcode b, used slot c, n and q:
 *   p_lm      = (1 - rho) (0.5 l + (m - l) 0.5 alpha) + rho a_i  for l, m = 0, 1, 2: the reference's mixture of genotype l of the first
 *               and m of the second sample (cmd_cram_demuxlet.cpp:616), diluted by the soup as dmx_engine_ambient dilutes a singlet;
 *   f_lm      = product over the pair's stored reads, in stored order, of pR (1 - p_lm) + pA p_lm (pR / pA as for dmx_engine_ambient);
 *   L_i       = sum_l sum_m gp[i][v1][l] gp[i][v2][m] f_lm, the float32 entries widened to float64 (their product is exact), l-major, m-minor;
 *   LL[b][c][n][q] = sum over b's pairs in ascending SNP order of log(L_i), the log being dmx_log.
 * No per-read renormalisation and no 1e-6 floor (:649): the values compare with dmx_engine_ambient's (alpha = 0 with a one-hot second
 * row IS the singlet profile of v1), not with the engine's doublet grid.  A pair with no stored read, or where either sample's gp row
 * is all zero, contributes nothing to that candidate; n_snp[b][c] / n_read[b][c] count the pairs / reads that did.  f_lm is kept in
 * range by exact power-of-two rescaling, one exponent per entry, carried into the log: pairs of hundreds of reads give the finite value
 * of the log-space sum.  Each (b, c, n, q) is one serial sum with no floating-point atomics and no cross-lane step: its bits depend on
 * b's data, (v1, v2), alpha and rho only — not on C, A, Q, the slot, the other candidates or what ran before — and a grid (rho or alpha)
 * split over two calls gives the same bits at the shared points.  Unused slots get zero rows.
 * Operations (binary64, every product and sum rounded on its own: no contraction; tests/contract_emul.cpp restates them and
 * tests/test_gpu_contract_bits.py compares the bits), entries in the order k = 3 l + m:
 *   p_lm      c_lm = 0.5 l + ((m - l) 0.5) alpha (the product with alpha and the sum rounded; the rest is exact);  om = 1 - rho,
 *             ra = rho a_i;  p_lm = om c_lm + ra,  q_lm = 1 - p_lm, rounded once;
 *   factor    as dmx_engine_ambient: e3 = err[bq] / 3,  t_lm = pR q_lm + pA p_lm,  f_lm = t_lm of the first stored read, then f_lm t_lm;
 *   weights   w_lm = gp[i][v1][l] gp[i][v2][m], exact;
 *   < 8 reads L = w_00 f_00, then L = L + w_lm f_lm in entry order (every product rounded);  lg = dmx_log(L);
 *   >= 8      after every eighth read (the pair's reads 8, 16, ...) every entry with 0 < f_lm < 2^-300 takes e = its exponent as frexp
 *             gives it, f_lm = ldexp(f_lm, -e), E_lm += e (from 0).  Per candidate E = max E_lm over the entries with w_lm != 0 and
 *             f_lm > 0;  t_lm = w_lm ldexp(f_lm, max(E_lm - E, -1100)) where w_lm != 0, else +0;  L = t_00, then L = L + t_lm in entry
 *             order;  lg = dmx_log(L), and when E != 0  lg = fma(E, DMX_LOG_LN2HI, fma(E, DMX_LOG_LN2LO, lg)).  A zero weight never
 *             zeroes a product here (no entry is shared between candidates).  Without an entry to take E from, L = 0;
 *   sum       LL[b][c][n][q] starts at +0 and takes lg pair by pair.
 * An L that is not a positive normal number goes to the runtime's log; on these paths that is L = 0 only, and the entry is -inf.
 * The call runs on the engine's stream,
 * synchronises it before returning (host inputs may be freed then), uses buffers of its own and leaves every other result of the
 * engine, the last dmx_engine_ambient profile included, as it was.
 * DMX_ERR_ARG: C or A outside [1, 8], Q outside [1, 256], alpha or grid outside [0, 1] or not strictly ascending, an a_i outside [0, 1],
 * a candidate that is neither unused nor two different samples in [0, V), n_cells / n_snps that do not match the staged pileup / the
 * genotype matrix.  DMX_ERR_STATE: no pileup or no genotypes yet.  DMX_ERR_NOMEM: the B x C x A x Q profile does not fit the free
 * device memory. */
typedef struct {
  int32_t n_cells;             /* = the staged pileup's n_cells */
  int32_t cand_memory;         /* DMX_MEM_HOST or DMX_MEM_DEVICE: where `cand` lives */
  const int32_t* cand;         /* [n_cells][n_cand][2] */
  int32_t n_cand;              /* C, 1..8 */
  int32_t n_alpha;             /* A, 1..8 */
  int32_t n_snps;              /* = the genotype matrix's n_snps */
  int32_t n_grid;              /* Q, 1..256 */
  const double* alpha;         /* [n_alpha] float64, strictly ascending, in [0, 1], HOST */
  const double* ambient;       /* [n_snps] float64 in [0, 1], HOST */
  const double* grid;          /* [n_grid] float64, strictly ascending, in [0, 1], HOST */
  int32_t reserved[4];         /* 0 */
} dmx_ambient_doublet_request;
typedef struct {
  double  kernel_ms;           /* HIP-event time of the last call's k_ambient_dbl */
  int64_t profile_bytes;       /* device bytes of the B x C x A x Q profile */
  int64_t n_used;              /* candidate slots in use */
  int32_t n_cells, n_cand, n_alpha, n_grid;
  int32_t reserved[4];
} dmx_ambient_doublet_info;
int dmx_engine_ambient_doublet(dmx_engine*, const dmx_ambient_doublet_request*);
/* Device->host copies of the last profile (any pointer may be NULL): ll[B][C][A][Q] f64, n_snp[B][C] / n_read[B][C] i32. */
int dmx_engine_get_ambient_doublet(dmx_engine*, double* ll, int32_t* n_snp, int32_t* n_read);
int dmx_engine_ambient_doublet_info(dmx_engine*, dmx_ambient_doublet_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Triplet profile (no counterpart in the reference): a barcode's base pair of donors with every sample of the pool
 * as a third donor, on the scale of dmx_engine_ambient / dmx_engine_ambient_doublet at rho = 0.  For up to C base slots per barcode,
 * base[b][s] = (v1, v2) with v1 = -1 = slot not used and otherwise 0 <= v1, v2 < V, v1 != v2, and share triples shares[t] = (w1, w2, w3),
 * t < T, over the staged pileup, the phred tables and the engine's genotype matrix gp (float32), for every barcode b, used slot s, t
 * and sample c in [0, V):
 *   p_lmn     = 0.5 (w1 l + w2 m + w3 n)  for l, m, n = 0, 1, 2, evaluated in that order in float64: the reference's ALT fraction
 *               (cmd_cram_demuxlet.cpp:613) with a third genome;
 *   f_lmn     = product over the pair's stored reads, in stored order, of pR (1 - p_lmn) + pA p_lmn (pR / pA as for dmx_engine_ambient);
 *   u_n       = sum_l sum_m gp[i][v1][l] gp[i][v2][m] f_lmn, the float32 entries widened to float64 (their product is exact), l-major, m-minor;
 *   L_c       = sum_n gp[i][c][n] u_n, n ascending;
 *   LL[b][s][t][c] = sum over b's pairs in ascending SNP order of log(L_c), the log being dmx_log.
 * No per-read renormalisation and no 1e-6 floor.  A pair with no stored read, or where the gp row of v1 or v2 is all zero, contributes
 * nothing to any c; a pair where the row of c is all zero contributes nothing to that c; n_snp[b][s][c] / n_read[b][s][c] count the
 * pairs / reads that did.  c = v1 and c = v2 are computed like any other column (a pair with one donor counted twice).  f_lmn is kept
 * in range by exact power-of-two rescaling, one exponent per entry, carried through u_n and L_c into the log (entries of zero weight do
 * not drive the scale): pairs of hundreds of reads give the finite value of the log-space sum.  Each (b, s, t, c) is one serial sum
 * with no floating-point atomics and no cross-lane step that depends on the rest of the call: its bits depend on b's data, (v1, v2),
 * the share triple, c and V only — not on C, T, the slot, the other slots, where `base` lives or what ran before.  Unused slots get
 * zero rows.  The call runs on the engine's stream, synchronises it before returning (host inputs may be freed then), uses buffers of
 * its own and leaves every other result of the engine, the ambient profiles included, as it was.
 * DMX_ERR_ARG: C or T outside [1, 8], a share outside [0, 1], a row with |w1 + w2 + w3 - 1| > 1e-12, two equal rows, a slot that is
 * neither unused nor two different samples in [0, V), n_cells / n_snps that do not match the staged pileup / the genotype matrix.
 * DMX_ERR_STATE: no pileup or no genotypes yet.  DMX_ERR_NOMEM: the B x C x T x V profile does not fit the free device memory. */
typedef struct {
  int32_t n_cells;             /* = the staged pileup's n_cells */
  int32_t base_memory;         /* DMX_MEM_HOST or DMX_MEM_DEVICE: where `base` lives */
  const int32_t* base;         /* [n_cells][n_base][2] */
  int32_t n_base;              /* C, 1..8 */
  int32_t n_shares;            /* T, 1..8 */
  int32_t n_snps;              /* = the genotype matrix's n_snps */
  int32_t reserved0;           /* 0 */
  const double* shares;        /* [n_shares][3] float64 in [0, 1], rows summing to 1 and pairwise different, HOST */
  int32_t reserved[4];         /* 0 */
} dmx_triplet_request;
typedef struct {
  double  kernel_ms;           /* HIP-event time of the last call's k_triplet */
  int64_t profile_bytes;       /* device bytes of the B x C x T x V profile */
  int64_t n_used;              /* base slots in use */
  int32_t n_cells, n_base, n_shares, n_samples;
  int32_t reserved[4];
} dmx_triplet_info;
int dmx_engine_triplet(dmx_engine*, const dmx_triplet_request*);
/* Device->host copies of the last profile (any pointer may be NULL): ll[B][C][T][V] f64, n_snp[B][C][V] / n_read[B][C][V] i32. */
int dmx_engine_get_triplet(dmx_engine*, double* ll, int32_t* n_snp, int32_t* n_read);
int dmx_engine_triplet_info(dmx_engine*, dmx_triplet_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Pileup composer (no counterpart in the reference): new barcodes made on the device from the reads of one or two
 * barcodes of the staged pileup, each read kept or dropped by a hash — in-silico doublets and thinned barcodes for power curves
 * (demuxlet_amd/simulate.py).  All integer; the result is defined bit for bit:
 *   mix64(z):  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  return z ^ z >> 31   (mod 2^64)
 *   for output o (id i = index_base + o), slot s in {0, 1}, SNP id n and read index r within the parent's pair:
 *     u = mix64(mix64(seed + 0x9E3779B97F4A7C15 * (2 i + s + 1)) + (n << 32 | r)) >> 32;   the read is kept iff u < keep[o][s].
 *   The hash sees the SNP id and the in-pair index only, so the result depends neither on the source's layout (dense or sparse) or
 *   nrd_width nor on the other rows of the recipe: a recipe composed in chunks (index_base) gives the same barcodes.
 *   A parent pair with stored reads survives iff it keeps at least one; a pair without stored reads (allele-2-only, see dmx_pileup)
 *   is decided as if it held one read of index 0.  Output o's pairs are the ascending union of the SNPs of both slots' surviving
 *   pairs; a pair's reads are slot 0's kept reads in stored order, then slot 1's.  parent[o][0] == parent[o][1] is allowed.
 *   The output is always sparse; its nrd_width is the source's, widened to the smallest of {1, 2, 4} that holds every merged count.
 * Three kernels (count, scan, fill), plain vector stores, no atomics: the bits do not depend on scheduling.  The call runs on the
 * engine's stream, synchronises it before returning and leaves every other result of the engine as it was.
 * DMX_ERR_ARG: a parent outside [0, n_cells) (slot 1: or -1 = none), keep > 2^32, n_out < 1 or > 2^24 (a longer recipe is composed in
 * chunks by index_base), a null array.  DMX_ERR_STATE: no staged
 * pileup, the staged pileup is this engine's own composed one, or _composed_pileup / _get_composed / _compose_info before a compose.
 * DMX_ERR_NOMEM: the composed pileup does not fit the free device memory. */
typedef struct {
  int32_t n_out;            /* output barcodes, 1 .. 2^24 */
  int32_t reserved0;        /* 0 */
  int64_t index_base;       /* output o is hashed as id index_base + o */
  const int32_t*  parent;   /* [n_out][2] cells of the staged pileup; slot 1 may be -1 (one parent); HOST */
  const uint64_t* keep;     /* [n_out][2] thresholds in [0, 2^32]: a read is kept iff its 32-bit hash < keep; 2^32 keeps all; HOST */
  uint64_t seed;
  int32_t reserved[4];      /* 0 */
} dmx_compose_request;
typedef struct {
  int64_t n_pairs, n_reads;           /* of the composed pileup */
  int64_t bytes_read, bytes_written;  /* algorithmic device bytes of the three kernels: the parents' pair_snp / pair_nrd twice (count and
                                         fill), the kept read bytes, the recipe and the counts; the composed arrays and the counts */
  double  count_ms, scan_ms, fill_ms; /* HIP-event times of k_compose<count>, k_compose_scan, k_compose<fill> */
  int32_t n_out, nrd_width;
  int32_t reserved[4];
} dmx_compose_info;
int dmx_engine_compose(dmx_engine*, const dmx_compose_request*);
/* The composed pileup as a DMX_MEM_DEVICE view owned by the engine (rd_* NULL: the caller attaches host counters where a consumer
 * needs them), for dmx_engine_set_pileup of ANOTHER engine or dmx_job.pileup; valid until the next compose / set_pileup / destroy. */
int dmx_engine_composed_pileup(dmx_engine*, dmx_pileup* out);
/* Device->host copies (any pointer may be NULL): cell_pair_off / cell_read_off [n_out + 1], pair_snp [n_pairs], pair_nrd [n_pairs] of
 * nrd_width bytes, reads [n_reads]. */
int dmx_engine_get_composed(dmx_engine*, int64_t* cell_pair_off, int64_t* cell_read_off, int32_t* pair_snp, void* pair_nrd, uint8_t* reads);
int dmx_engine_compose_info(dmx_engine*, dmx_compose_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * a6,a10..a14  finaliser and writers — replaces cmd_cram_demuxlet.cpp:465-527 (.single), :713-875 (.sing2/.pair/.best).
 *     Rows come out in ascending byte-wise barcode order (std::map<std::string,int32_t>, :472,:576); cells failing
 *     --min-total/--min-uniq/--min-snp are skipped (:480,:581); cells without any covered SNP get .single rows only
 *     (:592).  All arrays are HOST memory. */
typedef struct {
  int32_t n_cells, n_samples, n_alpha;
  const double* alpha;
  double  doublet_prior;
  int32_t min_total, min_uniq, min_snp;
  int32_t write_pair;
  const char* const* barcodes;     /* [n_cells] by cell id */
  const char* const* sample_ids;   /* [n_samples] */
  const int32_t *rd_totl, *rd_pass, *rd_uniq, *n_snp;   /* [n_cells] */
  const double* llks;              /* [n_cells][V]       (for .single) */
  const double* llk0s;             /* [n_cells] */
  const double* llksAB;            /* [n_cells][V][V][A] (for .sing2/.pair/.best) */
  const double* llks00;            /* [n_cells][A] */
  /* Optional tie arbiter: with the host pileup and genotype matrix present, grid entries within
   * tie_tol of a decision (top-2 singlets, best doublet) are re-evaluated on the host in the reference's exact
   * operation order with the host libm before the strict-< scans run, so DBL-a-b vs DBL-b-a follows the reference. */
  const dmx_pileup* tie_pileup;    /* NULL = no arbiter */
  const float*  tie_g;             /* [n_snps][V][3] */
  double  tie_tol;                 /* 0 = default 1e-7 */
} dmx_final_input;                 /* fixed layout since ABI 5: passed by pointer without a size member, it never grows */

int dmx_write_single(const dmx_final_input*, const char* path);                    /* <out>.single */
int dmx_write_doublet(const dmx_final_input*, const char* out_prefix);            /* <out>.sing2, <out>.best, [<out>.pair] */
/* The same <out>.sing2 and <out>.best from the per-cell records of the device-side reduction (dmx_engine_get_sing,
 * dmx_engine_get_doublet's summary and llks00) instead of the full grid: what a multi-GPU run gathers to rank 0.
 * in->llksAB is ignored; in->write_pair must be 0 (the .pair rows need the grid).  With in->tie_pileup the order of
 * the two samples of an alpha = 0.5 best doublet is arbitrated exactly.  Barcodes K3 flagged as near-ties
 * (another sample pair, another alpha or another singlet within 1e-7 of a decision: duplicate samples, a handful of covered SNPs)
 * need more than their record: pass their grids to dmx_write_doublet_summary_grids; without a grid but with in->tie_pileup the barcode's
 * WHOLE grid is re-evaluated on the host in the reference's operation order (exact, pairs x V x V x A host log() calls for that barcode;
 * refused with DMX_ERR_ARG beyond 2e9 such calls in one job — pass the grids); with neither, the device's own choice among the near-tied
 * candidates is printed (each within 1e-7 of the reference's best).  A barcode with DMX_CELL_NEAR_RULE has the entries of the BEST rule
 * re-evaluated when in->tie_pileup is there (no grid needed). */
int dmx_write_doublet_summary(const dmx_final_input*, const double* sing, const dmx_cell_summary* summary, const char* out_prefix);
/* (ABI 7) The same with cell_grid[n_cells]: pointers to single cells' llksAB[V][V][A] (NULL entries = none; a NULL array = none =
 * dmx_write_doublet_summary).  A barcode whose K3 record carries DMX_CELL_NEAR_DOUBLET / _NEAR_SINGLET is decided from its grid
 * (dmx_engine_get_cell_grids fetches exactly those), with the tie arbiter re-evaluating the contenders as dmx_write_doublet does. */
int dmx_write_doublet_summary_grids(const dmx_final_input*, const double* sing, const dmx_cell_summary* summary,
                                    const double* const* cell_grid, const char* out_prefix);
/* For consumers of the K3 records themselves: turn every DMX_CELL_ORDER_RESOLVABLE record among summary[0..n) into a certified one
 * by asking this host's libm for the one or two log() values the device left open (the writers above do the same internally).
 * Returns the number of records that stay unresolved (>= 0), or a negative dmx_status. */
int dmx_resolve_tie_order(dmx_cell_summary* summary, int64_t n);

/* Diagnostics: evaluate the device's log() replacement (dmx_log, csrc/dmx_log.hpp) on n host doubles. Used by the tests
 * to show the device function performs exactly the IEEE operation sequence whose accuracy is measured on the host. */
int dmx_debug_device_log(const double* x, double* y, int64_t n, int32_t device);
int dmx_debug_device_log2(const double* x, double* y, int64_t n, int32_t device);   /* dmx_log2: the doublet kernels' log (256 bins, ABI 6) */
int dmx_debug_device_log2_lite32(const double* x, double* y, int64_t n, int32_t device); /* (ABI 8, appended in round 6) FAST's second phase-2 log: split 32-bin table (conflict-free LDS reads), degree-5 near-minimax tail — 8 FP64 instructions, |error| <= 1.2e-15 absolute (csrc/dmx_log.hpp) */
int dmx_debug_device_log2_lite(const double* x, double* y, int64_t n, int32_t device);   /* (ABI 7) DMX_MODE_FAST's phase-2 log: dmx_log2's table, series cut after r^4/4 — 6 FP64 instructions, |error| <= 6e-15 absolute, unbiased (csrc/dmx_log.hpp) */
int dmx_debug_device_log2_mirror(const double* x, const double* xm, double* y, double* ym, int64_t n, int32_t device);   /* (ABI 8, appended) dmx_log2 of the mirrored pairs (x[i], xm[i]) — two sums of the same terms in two orders — through the device functions of the STRICT unordered-pair doublet kernels: the mirror takes the primary's table entry when the high words agree from bit 11 up, its own otherwise (csrc/dmx_log.hpp); y[i], ym[i] = dmx_debug_device_log2's bits for x[i], xm[i].  Normal positive arguments. */
/* Diagnostics: the device's log() ceiling, measured by a register-resident microkernel (no memory traffic): which = 0 the
 * kernels' dmx_log, which = 1 ocml's log().  bench.py reports both next to the kernels' achieved log rate. */
int dmx_debug_log_rate(int32_t which, int32_t iters, int32_t device, double* logs_per_second);   /* which: 0 dmx_log, 1 ocml log(), 2 dmx_log2 */
/* Diagnostics: q[i] = a[i] / b[i] through the kernels' shared-reciprocal division (must equal IEEE division bit for bit
 * for 2^-700 < a,b < 2^700). */
int dmx_debug_device_div(const double* a, const double* b, double* q, int64_t n, int32_t device);

/* Diagnostics (host evaluation of the code the device runs): the double-double logarithm behind the tie-order certificate
 * (csrc/dmx_log.hpp, DESIGN.md "Ties").  hi[i] + lo[i] = log(x[i]) to ~2^-75; [t_lo[i], t_hi[i]] = the doubles a libm with
 * < 0.53 ulp error can return for log(x[i]) (one double, or the two neighbours of a rounding midpoint). */
int dmx_debug_log_dd(const double* x, double* hi, double* lo, double* t_lo, double* t_hi, int64_t n);

/* ------------------------------------------------------------------------------------------------------------------
 * One call for the whole of cmd_cram_demuxlet.cpp:390-881: store + genotype matrix + options in, four files out. */
typedef struct {
  dmx_store*   store;
  const float* g;                  /* [n_snps][V][3], HOST */
  int32_t      n_samples;
  const char* const* sample_ids;
  int32_t      n_alpha;  const double* alpha;
  double       doublet_prior;
  int32_t      min_total, min_uniq, min_snp, write_pair;
  const char*  out_prefix;
  int32_t      device;
  int32_t      arbiter;            /* 1 = run the tie arbiter (default in the CLI) */
  int32_t      n_gpus;             /* 0 or 1: one GPU (`device`).  N > 1: devices (device + i) mod (visible devices).  The byte-wise
                                      sorted barcodes are cut into contiguous ranges of equal work — at least one per GPU, four for jobs
                                      worth overlapping, more when a range's doublet grid would exceed the byte budget (4 GiB, or a sixth of
                                      the free device memory) — which go through the GPUs in waves.  With several waves every GPU runs two
                                      engines (own HIP stream each) that alternate: the H2D of wave w + 2 overlaps the kernels of wave w + 1
                                      while the host arbitrates, formats and appends the rows of wave w.  Barcodes are independent
                                      (cmd_cram_demuxlet.cpp:576): no collective. */
  int32_t      mode;               /* DMX_MODE_STRICT (0: the default of this struct, of the Python binding and of the `demuxlet`
                                      binary) or DMX_MODE_FAST (`demuxlet --fast`) */
  /* Optional (ABI 2): a pileup that is already frozen (sparse or dense layout) instead of `store` (then NULL), with its barcodes by
   * cell id — what a caller that builds the CSR itself hands over (tools/e2e_bench.cpp, the benchmarks).  memory = DMX_MEM_HOST, or
   * (ABI 6) DMX_MEM_DEVICE: the five arrays live in the HBM of `device` (n_gpus <= 1), the rd_* counters stay host memory.  Nothing is
   * then sliced or copied on the host: a range of consecutive cells is a view of the caller's arrays, any other range is gathered
   * on the device, and the barcodes the tie arbiter walks (near-tie flags, an open tie-order certificate) have their pieces fetched. */
  const dmx_pileup*  pileup;
  const char* const* barcodes;
  /* Optional (ABI 2): wall-clock seconds of the stages of this call, written on return (NULL = not wanted). */
  struct dmx_job_timing* timing;
} dmx_job;
typedef struct dmx_job_timing {
  double freeze_s;                 /* dmx_store_freeze */
  double setup_s;                  /* engine creation, genotype upload, class detection */
  double stage_s;                  /* slicing the CSR into ranges + H2D (host time, all ranges) */
  double wait_s;                   /* host blocked on the GPUs (kernels not hidden behind host work) + D2H of the results */
  double write_s;                  /* tie arbiter + row formatting + file writes (all ranges) */
  double total_s;
  double kernel_ms;                /* sum over ranges of the K1 + K2 + K3 HIP-event times (device time, all engines) */
  int32_t n_ranges, n_engines, n_cells_grid_fetched;
  int32_t n_cells_single;          /* barcodes that passed --min-total / --min-uniq / --min-snp: the droplets of cmd_cram_demuxlet.cpp:480-524 (ABI 6; was `reserved`) */
} dmx_job_timing;
int dmx_demuxlet_run(const dmx_job*);
/* Creates the HIP contexts of devices (device + i) mod (visible devices), i < n_gpus (n_gpus <= 0: one), and returns.  Optional: the first
 * job of a process otherwise pays this (0.12-0.13 s) inside dmx_demuxlet_run; a caller that still has host work to do (the `demuxlet`
 * binary: the BAM x VCF scan, cmd_cram_demuxlet.cpp:195-338) calls it on a thread of its own first.  Thread-safe. */
int dmx_device_warm_up(int32_t device, int32_t n_gpus);

/* ------------------------------------------------------------------------------------------------------------------
 * Donor shares of a read pool (no counterpart in the reference; appended, DMX_ABI_VERSION stays 8).  Every stored
 * read of a group of barcodes is an independent draw from a mixture of the V donors: which donors, in what proportions, make up the pool.
 * Inputs: the staged pileup, the phred tables, the engine's genotype matrix gp[S][V][3] (float32), group[B] with entries in [-1, G)
 * (-1 = barcode not used) and shares w[G][V], non-negative, each row summing to 1 within 1e-12.
 *   d[i][v]   = (gp1 / 2 + gp2) / ((gp0 + gp1) + gp2), in float64 from the float32 entries.  A SNP where a donor's row does not sum to a
 *               positive finite number is INVALID: its pairs are skipped for every group; dmx_census_info counts these SNPs.
 *   A_i(w)    = sum over v, ascending, of w[v] d[i][v]; every product and sum is rounded on its own (no fused multiply-add).
 *   P_r       = pR (1 - A_i) + pA A_i for a stored read, pR = allele 0 ? mat[bq] : err[bq] / 3, pA = allele 1 ? mat[bq] : err[bq] / 3
 *               (as for dmx_engine_ambient).  Reads of allele 2 are not stored (see dmx_pileup): they are skipped and not counted.
 *   LL[g]     = sum over the reads of group g of log P_r, the log being dmx_log;
 *   acc[g][v] = sum over the pairs of group g of (1 - d[i][v]) sR + d[i][v] sA, sR = sum over the pair's reads of pR / P_r, sA = sum of
 *               pA / P_r (IEEE divisions).  Every term is non-negative.
 *   n_read[g] / n_pair[g] = the reads / pairs counted (pairs with a stored read at a valid SNP).
 * The EM image of w is w'[v] = w[v] acc[v] / N, N = n_read[g]; gap[g] = N (max_v acc[v] / N - 1).  Because sum_v w[v] acc[v] = N and LL is
 * concave in w, LL(w_MLE) - LL(w) <= gap: the gap is the stopping rule.  A group without a counted read has acc = 0, LL = 0, gap = 0.
 * Summation plan (no floating-point atomics; it depends on the pileup, the group's own members and V only): the barcodes of a group in
 * ascending cell id are cut into chunks of 4.  Within a chunk, barcodes in that order, pairs in stored order, 64 pairs (a tile) at a time:
 * acc[v] adds one term per pair in that order (for V <= 32, with Vq the power of two >= V and n = 64 / Vq: n running sums, sum s taking
 * the tile's pairs s, s + n, ..., added in order at the chunk's end); each of the tile's 64 positions keeps its own running LL over the
 * chunk, and the 64 are added in position order at the chunk's end.  A group's chunks are folded in order into eight accumulators (chunk c into c mod 8),
 * which are added as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)).  Therefore a repeat gives the same bits; a group evaluated alone gives
 * the same bits as among other groups; a device `group` gives the same bits as a host one; the stream and earlier calls do not matter;
 * nrd_width does not matter.  (The dense and the sparse layout of one pileup tile a barcode's pairs differently: same values to rounding.)
 *
 * dmx_engine_census_step: one device pass at w (k_census_dosage once, then k_census_step and k_census_fold); any output may be NULL.
 * dmx_engine_census: the loop inside the library, from w0 (NULL = uniform 1 / V).  Per pass only G (V + 3) doubles cross to the host.
 *   Plain EM (accelerate = 0): w <- w'.  SQUAREM (accelerate != 0), one cycle from w0: a pass at w0 gives w1, a pass at w1 gives w2;
 *   r = w1 - w0, u = (w2 - w1) - r, steplength a = -|r| / |u| (Euclidean norms; -1 when |u| = 0), clamped to <= -1;
 *   x = w0 - 2 a r + a^2 u; while a component of x is negative and a < -1, a <- (a - 1) / 2, taken as -1 once within 1e-9 of it (at a = -1, x = w2); x is clipped at 0 and
 *   divided by its sum; a pass at x gives the stabilising step x' and LL(x); the next cycle starts from x', or from w2 when LL(x) is not
 *   finite or below LL(w1).
 *   After every pass, at the point just evaluated: a group stops when its LL is finite and gap <= tol (converged = 1), or when it has
 *   taken max_steps passes (converged = 0); it returns that point with its LL and gap.  A stopped group is frozen: its wavefronts
 *   return at once in later passes and its results stay.  A group without a counted read returns its input w, ll = 0, gap = 0,
 *   converged = 1 after one pass.  tol <= 0 selects 1e-4 (LL units), max_steps <= 0 selects 2000.
 * Both calls run on the engine's stream, synchronise it before returning (host inputs may be freed then), use buffers of their own and
 * leave every other result of the engine as it was.
 * DMX_ERR_ARG: G outside [1, 1024], V above 1024, n_samples that is not the engine's, group[b] outside [-1, G), a w entry that is negative
 * or not finite, a row sum off 1 by more than 1e-12, n_cells that does not match the staged pileup, a null group (B > 0) or w.
 * DMX_ERR_STATE: no pileup or no genotypes yet (or dmx_engine_get_census / _census_info before a call).  DMX_ERR_NOMEM: the S x V dosage
 * table or the chunk partials do not fit the free device memory. */
typedef struct {
  int32_t n_cells;             /* = the staged pileup's n_cells */
  int32_t group_memory;        /* DMX_MEM_HOST or DMX_MEM_DEVICE: where `group` lives */
  const int32_t* group;        /* [n_cells], -1 = not used */
  int32_t n_groups;            /* G, 1..1024 */
  int32_t n_samples;           /* V = the engine's n_samples, <= 1024 */
  const double* w;             /* [G][V] float64, HOST */
  double*  acc;                /* out [G][V], HOST (NULL = not wanted) */
  double*  ll;                 /* out [G] */
  double*  gap;                /* out [G] */
  int64_t* n_read;             /* out [G] */
  int64_t* n_pair;             /* out [G] */
  int32_t reserved[4];         /* 0 */
} dmx_census_step_request;
typedef struct {
  int32_t n_cells;             /* = the staged pileup's n_cells */
  int32_t group_memory;        /* DMX_MEM_HOST or DMX_MEM_DEVICE */
  const int32_t* group;        /* [n_cells], -1 = not used */
  int32_t n_groups;            /* G, 1..1024 */
  int32_t n_samples;           /* V = the engine's n_samples, <= 1024 */
  const double* w0;            /* [G][V] start, HOST; NULL = uniform */
  double  tol;                 /* stop at gap <= tol; <= 0: 1e-4 */
  int32_t max_steps;           /* passes per group at most; <= 0: 2000 */
  int32_t accelerate;          /* 0 = plain EM, otherwise SQUAREM */
  int32_t reserved[4];         /* reserved[0] = gap_on_support (see the census uncertainty block below); the others 0 */
} dmx_census_request;
typedef struct {
  double  kernel_ms;           /* HIP-event time of the last pass: k_census_step + k_census_fold */
  double  dosage_ms;           /* ... and of the last call's k_census_dosage */
  int64_t dosage_bytes;        /* device bytes of d[S][V] */
  int64_t partial_bytes;       /* device bytes of the chunk partials */
  int32_t n_steps;             /* passes the last call ran (dmx_engine_census_step: 1) */
  int32_t n_invalid_snps;
  int32_t n_groups, n_chunks, n_cells, n_samples;
  int32_t reserved[4];
} dmx_census_info;
int dmx_engine_census_step(dmx_engine*, const dmx_census_step_request*);
int dmx_engine_census(dmx_engine*, const dmx_census_request*);
/* The last dmx_engine_census result (any pointer may be NULL): w[G][V], ll[G], gap[G] f64; n_steps[G], converged[G] i32; n_read[G],
 * n_pair[G] i64. */
int dmx_engine_get_census(dmx_engine*, double* w, double* ll, double* gap, int32_t* n_steps, int32_t* converged, int64_t* n_read,
                          int64_t* n_pair);
int dmx_engine_census_info(dmx_engine*, dmx_census_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Census uncertainty: the observed information of the shares and the per-barcode scores (appended,
 * DMX_ABI_VERSION stays 8).  Inputs as for dmx_engine_census_step.  At shares w, the step's quotients of a stored read r of pair
 * (barcode b, SNP i) are tR = pR / P_r and tA = pA / P_r (the same IEEE divisions as in the step, on the same A_i and P_r).
 *   Per pair: sRR = sum_r tR tR, sRA = sum_r tR tA, sAA = sum_r tA tA, reads in stored order (and the step's sR = sum tR, sA = sum tA).
 *   With e_v = 1 - d[i][v], the observed information of group g (minus the Hessian of LL in w, unconstrained) is
 *     H[g][v][u] = sum over the pairs of g of ((e_v e_u) sRR + (e_v d_u + d_v e_u) sRA) + (d_v d_u) sAA,  for v <= u;
 *   every product and sum is rounded on its own, every term is non-negative, and the lower triangle is a copy of the upper.
 *   score[b][v] = sum over the pairs of barcode b of e_v sR + d_v sA: the step's acc kept per barcode, so the barcodes of a group sum to
 *   the group's acc (to rounding).  n_read_b[b] = the reads of b counted.  Barcodes with group -1 have a zero row and 0 reads.
 *   Identities: sum_u H[g][v][u] w[g][u] = acc[g][v], and w' H w = N = n_read[g] (both to rounding).
 * Summation plan: the step's chunks of 4 barcodes.  The E = V (V + 1) / 2 upper-triangle entries, numbered row-major, are cut into blocks
 * of 2048; one wavefront per (chunk, block) adds, for each of its entries, one term per pair: barcodes in chunk order, pairs in stored
 * order (a pair without a counted read adds +0).  A group's chunk partials are folded as the step's are: chunk c into accumulator c mod 8,
 * then ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)).  A score row adds one term per pair of the barcode in stored order (for V <= 32 with the
 * step's n = 64 / Vq running sums per tile position class, added in order at the barcode's end).  So a repeat, a group alone or among
 * others, a host or a device `group`, nrd_width and earlier calls give the same bits; a barcode's score row depends on its own pairs and
 * its w row only.  acc, ll, n_read and n_pair come from a dmx_engine_census_step pass inside the call and carry its bits.
 * Every group given is computed (nothing is frozen).  The call runs on the engine's stream, synchronises it before returning, uses buffers of
 * its own for H, the scores and their partials and leaves every other result of the engine, dmx_engine_get_census and
 * dmx_engine_census_info included, as it was.
 * DMX_ERR_ARG: as dmx_engine_census_step, and V > 128 (the chunk partials, chunks x E doubles, would not fit for a large pileup).
 * DMX_ERR_STATE: as dmx_engine_census_step; dmx_engine_census_fisher_info before a call.  DMX_ERR_NOMEM: the partials, H and the score
 * rows do not fit the free device memory.
 *
 * gap_on_support (dmx_census_request.reserved[0]): 0 keeps every bit of dmx_engine_census.  Non-zero: after each pass the driver takes
 * gap[g] = N (max over {v : w0[g][v] > 0} of acc[v] / N - 1), computed on the host from the pass's acc, instead of the maximum over all
 * donors.  EM and SQUAREM keep a zero share at zero, so this is the duality gap of the problem constrained to the support of the start;
 * without it a refit with a donor held at 0 whose acc stays above N never reaches gap <= tol.  With w0 = NULL (uniform) every donor is
 * in the support. */
typedef struct {
  int32_t n_cells;             /* = the staged pileup's n_cells */
  int32_t group_memory;        /* DMX_MEM_HOST or DMX_MEM_DEVICE: where `group` lives */
  const int32_t* group;        /* [n_cells], -1 = not used */
  int32_t n_groups;            /* G, 1..1024 */
  int32_t n_samples;           /* V = the engine's n_samples, <= 128 */
  const double* w;             /* [G][V] float64, HOST */
  double*  H;                  /* out [G][V][V], HOST (NULL = not wanted, as every output) */
  double*  score;              /* out [n_cells][V] */
  int64_t* n_read_b;           /* out [n_cells] */
  double*  acc;                /* out [G][V] */
  double*  ll;                 /* out [G] */
  int64_t* n_read;             /* out [G] */
  int64_t* n_pair;             /* out [G] */
  int32_t reserved[4];         /* 0 */
} dmx_census_fisher_request;
typedef struct {
  double  kernel_ms;           /* HIP-event time of k_census_fisher + k_census_fisher_fold */
  int64_t partial_bytes;       /* device bytes of the chunk partials: n_chunks x n_entries doubles */
  int32_t n_groups, n_chunks;
  int32_t n_blocks;            /* entry blocks of 2048 per chunk: the grid is n_chunks x n_blocks wavefronts */
  int32_t n_entries;           /* V (V + 1) / 2 */
  int32_t n_cells, n_samples;
  int32_t reserved[4];
} dmx_census_fisher_info;
int dmx_engine_census_fisher(dmx_engine*, const dmx_census_fisher_request*);
int dmx_engine_census_fisher_info(dmx_engine*, dmx_census_fisher_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Anchored doublet search (appended, DMX_ABI_VERSION stays 8): the doublet stage for panels whose grid
 * llksAB[V][V][A] does not fit or takes too long.  It evaluates the entries of that grid in which one donor is an ANCHOR (one of the
 * barcode's T best singlets, or a sample the caller names) or the second donor is sample 0, about (2T + 1) V (A - 1) + V A entries per
 * barcode instead of V V A, and derives K3's record from them.
 * Arithmetic: the STRICT contract of DESIGN.md section 4, whatever the engine's mode — the reference's operation order, no contraction,
 * IEEE division, the per-read renormalisation with one maximum across all alphas and the 1e-6 floor (cmd_cram_demuxlet.cpp:600-663),
 * nine-term l-major sums from 0.0 (:675-681), dmx_log2, and one serial sum per entry over the barcode's pairs in ascending SNP order.
 * Every evaluated entry is bit for bit the entry of dmx_engine_run_doublet's grid in DMX_MODE_STRICT.
 * For barcode b, V samples, alphas alpha[0..A), A >= 2:
 *   c0[j][n]   = llksAB[j][0][n], every j < V and n < A.  sing[j] = c0[j][0] is the singlet column that .sing2 prints, computed as the
 *                reference computes it: the pair (j, sample 0) at alpha[0], whatever that value is (:746-770).  The entries n >= 1 are
 *                what LLK10 / LLK20 read (:824-825); c0[0][n] is the diagonal entry.
 *   llks00[n]  :699-709.
 *   anchors    a_1 .. a_T: the caller's anchors[b][t] (-1 = slot not used; the used ids of a row pairwise different), or, with
 *                anchors == NULL, chosen on the device: T times the first maximum of sing[] in ascending j among the samples not yet
 *                chosen (the first-maximum rule of :746-758, repeated).
 *   pairs[t][k][0][n-1] = llksAB[a_t][k][n] and pairs[t][k][1][n-1] = llksAB[k][a_t][n] for every k < V, k != a_t, and n >= 1; the
 *                slots k = a_t and the rows of unused anchors are 0.
 *   D_b        = {(j, k, n) : n >= 1, j != k, and (j is an anchor, or k is an anchor, or k = 0)}: the evaluated doublet entries.
 * Record (dmx_cell_summary): n_pairs; i_sing1, i_sing2, sing_llk1, sing_llk2 from sing[] as K3 does; (j_best, k_best, n_best) the first
 * maximum over D_b in the reference's scan order (j, then k, then n ascending, strict <, :799-814), an entry reachable through two
 * anchors counting once; llk12; llk1 = sing[j_best], llk2 = sing[k_best], llk10 = c0[j_best][n_best], llk20 = c0[k_best][n_best];
 * llk00_0, llk00_best; max_llk = the maximum over sing[] and D_b (the entries [j][k != 0][0] that the reference also scans are not
 * evaluated: DMX_MODE_FAST's convention; every printed quantity is a ratio in which max_llk cancels); sum_single = :726 over all V;
 * sum_double = :731 over D_b with the reference's weights unchanged (/ V / (V - 1) / (A - 1), and / 2 at alpha = 0.5): the omitted pairs
 * count as 0, so PRB.DBL is a LOWER BOUND of the reference's.  DMX_CELL_NEAR_DOUBLET / _NEAR_SINGLET / _NEAR_RULE follow K3's rules over
 * the evaluated entries; DMX_CELL_ORDER_CERTIFIED / _RESOLVABLE are never set and llk_ab .. ev_t_ba are 0.  A barcode without pairs gets
 * the record K3 writes for it (an all-zero grid).
 * Determinism: an entry's bits depend on b's data, (j, k, n), the alpha grid, the rows of j, k and sample 0 and V only — not on T, the
 * anchor's rank, where `anchors` lives, nrd_width, the pileup's layout, the other barcodes, how entries are packed into wavefronts or
 * what ran before.  No floating-point atomics.
 * The call runs on the engine's stream and synchronises it, uses buffers of its own, never allocates the grid and leaves every other
 * result of the engine as it was.
 * DMX_ERR_ARG: V < 2 or A < 2 (or A > 64, V*V*A >= 2^31); n_anchor outside [1, 8] or above V; an anchor outside [-1, V); a repeated
 * anchor in a row; n_cells that does not match the staged pileup; a genotype matrix with a row that is not finite, non-negative and
 * somewhere above 1e-30 (run the full grid, which has the fix-up pass for such a matrix: this pass has none).
 * DMX_ERR_STATE: no pileup or no genotypes yet; dmx_engine_get_anchored / _anchored_info before any anchored call.
 * DMX_ERR_NOMEM: the results do not fit the free device memory (checked before anything is allocated). */
typedef struct {
  int32_t n_cells;             /* = the staged pileup's n_cells */
  int32_t n_anchor;            /* T, 1..8, <= V */
  int32_t anchor_memory;       /* DMX_MEM_HOST or DMX_MEM_DEVICE: where `anchors` lives */
  int32_t reserved0;           /* 0 */
  const int32_t* anchors;      /* [n_cells][T], -1 = unused; NULL = chosen on the device */
  int32_t reserved[4];         /* 0 */
} dmx_anchored_request;
typedef struct {
  double  col_ms;              /* HIP-event time of k_anchor_col and the anchor choice (k_anchor_select, or the upload of the caller's) */
  double  pair_ms;             /* ... of k_anchor_pair */
  double  reduce_ms;           /* ... of k_anchor_reduce */
  int64_t result_bytes;        /* device bytes of anchors, c0, pairs, llks00 and the records */
  int64_t n_entries;           /* entries evaluated: B (V A + A) + used anchors x (V - 1) x 2 x (A - 1) */
  int32_t n_cells, n_samples, n_alpha, n_anchor;
  int32_t reserved[4];
} dmx_anchored_info;
int dmx_engine_doublet_anchored(dmx_engine*, const dmx_anchored_request*);
/* Device->host copies of the last result (any pointer may be NULL): anchors[B][T] i32, c0[B][V][A], pairs[B][T][V][2][A-1],
 * llks00[B][A] f64, summary[B]. */
int dmx_engine_get_anchored(dmx_engine*, int32_t* anchors, double* c0, double* pairs, double* llks00, dmx_cell_summary* summary);
int dmx_engine_anchored_info(dmx_engine*, dmx_anchored_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Empirical-Bayes priors (appended, DMX_ABI_VERSION stays 8): the donor shares pi[V] of the pool's CELLS and the
 * doublet rate d, fitted by EM from the doublet grid llksAB[B][V][V][A] that dmx_engine_run_doublet leaves on the device (either mode:
 * DMX_MODE_FAST mirrors the alpha = 0.5 entries), and the per-barcode posteriors under those priors.
 * Model, for barcode b with L[j][k][n] = llksAB[b][j][k][n]: the USED entries are S_j = L[j][0][0] (the singlet column .sing2 prints)
 * and D_jkn = L[j][k][n] for j != k, n >= 1; the entries [j][k != 0][0] and the diagonal at n >= 1 are never read into a result.  A droplet
 * holds two cells with probability d, else one; cells are independent draws from pi; a homotypic doublet has the singlet's
 * likelihood; a doublet's alpha is uniform over the grid's A - 1 values:
 *   w_S(j) = (1 - d) pi_j + d pi_j^2,   w_D(j,k,n) = d pi_j pi_k / (A - 1),
 *   E_b = sum_j w_S(j) exp(S_j) + sum_{j != k, n >= 1} w_D(j,k,n) exp(D_jkn),   LL = sum_b log E_b.
 * Responsibilities r = w exp(.) / E_b; h_j = r_S(j) d pi_j / ((1 - d) + d pi_j) is the homotypic part of a singlet-like one.  A term whose
 * weight is exactly 0 or whose entry is -inf is exactly 0.  One step at (pi, d) gives, over the included barcodes,
 *   N_j = sum_b [ r_S(j) + h_j + sum_{k,n} r_D(j,k,n) + sum_{k,n} r_D(k,j,n) ],  hom = sum_b sum_j h_j,  het = sum_b sum r_D,  LL,
 * and the M-step pi'_j = N_j / sum_j N_j, d' = min(1, (hom + het) / B_in).  fix_pi / fix_d keep pi / d.
 * A barcode is INCLUDED unless mask[b] == 0 (DMX_PRIOR_MASKED) or it is BAD (DMX_PRIOR_BAD): a NaN or +inf among its used entries, or no
 * term above zero (every used entry -inf or of weight 0).  Flagged barcodes get rows and records of zeros and count nowhere.
 * Per-barcode row (prior_step): N contributions [V] | homotypic mass | heterotypic mass | log E_b.
 * Per-barcode record (prior_call): dmx_prior_call below.
 * Sum order of the fold (section 12's convention): the included barcodes in ascending id are cut into chunks of 64; a chunk's rows are
 * added in barcode order from 0.0, the chunk partials in ascending chunk order from 0.0.  No floating-point atomics: a barcode's row and
 * record depend on its own grid, pi, d, V and A only; N, hom, het, LL, pi', d' on the included rows only — not on launch geometry, the
 * stream, earlier calls, or where the grid lives.
 * pi given by the caller is divided by its sum (ascending j) first.  Limits: V >= 2, A >= 2, V A <= 4096 (the LDS holds the column
 * slots of a barcode: DESIGN.md section 25), V V A < 2^31; n_samples / n_alpha are the engine's.
 * Every call runs on the engine's stream and synchronises it, uses buffers of its own and leaves every other result as it was.
 * Among themselves: a refused call (DMX_ERR_ARG for sizes, pi or d; DMX_ERR_STATE; DMX_ERR_NOMEM) leaves the last step's, fit's and call's
 * results readable; dmx_engine_prior_call never touches a step's rows or flags (a record carries its own flag); dmx_engine_prior_fit
 * overwrites the step's rows, after which dmx_engine_get_prior_step is DMX_ERR_STATE, as it is after a step without an included barcode.
 * DMX_ERR_STATE: grid == NULL before dmx_engine_run_doublet; a getter before its call.  DMX_ERR_ARG: sizes that do not match or exceed
 * the limits; pi not finite, negative or summing to 0; d outside [0, 1]; no included barcode (B_in == 0).  DMX_ERR_NOMEM: the buffers do
 * not fit the free device memory (checked before anything is allocated). */
enum { DMX_PRIOR_MASKED = 1, DMX_PRIOR_BAD = 2 };
typedef struct {
  int32_t n_cells;             /* B: the staged pileup's with grid == NULL, else the caller's grid's */
  int32_t n_samples, n_alpha;  /* = the engine's V and A */
  int32_t grid_memory;         /* DMX_MEM_HOST or DMX_MEM_DEVICE: where `grid` lives (ignored with grid == NULL) */
  const double* grid;          /* [B][V][V][A], or NULL = the engine's llksAB of the last dmx_engine_run_doublet */
  const uint8_t* mask;         /* host [B], 0 = leave out; NULL = barcodes with n_pairs > 0 (engine's grid) / all barcodes (caller's grid) */
  const double* pi0;           /* fit: host [V] start, NULL = uniform */
  double  d0;                  /* fit: start (with fix_d: the value held) */
  double  tol;                 /* fit: stop once LL gained less than tol * B_in in an iteration; <= 0: run max_iter iterations */
  int32_t max_iter;            /* fit: >= 1 */
  int32_t fix_pi, fix_d;       /* fit: hold the shares / the rate */
  int32_t reserved[5];         /* 0 */
} dmx_prior_request;
typedef struct {
  double  log_e;               /* log E_b */
  double  p_sng, p_het, p_hom; /* sum_j (r_S(j) - h_j), sum r_D, sum_j h_j: they add up to 1 */
  double  p_sng1, p_sng2;      /* the two largest r_S(j) (first maximum wins; second = first maximum of the rest, as K3 does) */
  double  p_dbl1;              /* responsibility of the largest doublet term */
  int32_t i_sng1, i_sng2;
  int32_t j_dbl, k_dbl, n_dbl; /* first maximum of w_D exp(D) in the scan order j, k, n ascending, strict <; -1 without a term above zero */
  int32_t flag;                /* 0, DMX_PRIOR_MASKED or DMX_PRIOR_BAD */
} dmx_prior_call;
typedef struct {
  double  estep_ms;            /* HIP-event time of the last k_prior_estep */
  double  fold_ms;             /* ... of the last fold (k_prior_rank, k_prior_fold_chunk, k_prior_fold) */
  double  call_ms;             /* ... of the last k_prior_estep<call> */
  double  fit_ms;              /* sum of estep_ms + fold_ms over the last fit's iterations */
  int64_t bytes_per_iter;      /* grid bytes one iteration reads from memory (B V V A 8: the second pass is counted as cache hits) */
  int32_t n_iter;              /* iterations of the last fit (its final evaluation not counted) */
  int32_t n_cells, n_samples, n_alpha, waves_per_block;
  int32_t reserved[3];
} dmx_prior_info;
/* One E + M at (pi[V], d).  Results: dmx_engine_get_prior_step. */
int dmx_engine_prior_step(dmx_engine*, const dmx_prior_request*, const double* pi, double d);
/* Any pointer may be NULL: N[V], hom, het, ll, b_in, pi_next[V], d_next, rows[B][V + 3], flags[B] (uint8). */
int dmx_engine_get_prior_step(dmx_engine*, double* N, double* hom, double* het, double* ll, int32_t* b_in, double* pi_next, double* d_next,
                              double* rows, uint8_t* flags);
/* The EM loop from (pi0, d0): per iteration one step and V + 3 doubles read back; iteration t's LL_t and d_t (the values it was
 * evaluated at) are recorded; it stops after the iteration whose LL_t - LL_{t-1} < tol * B_in (converged) or after max_iter.  One more
 * E-step at the final (pi, d) then gives the reported N, hom, het and LL.  Results: dmx_engine_get_prior_fit. */
int dmx_engine_prior_fit(dmx_engine*, const dmx_prior_request*);
/* Any pointer may be NULL: pi[V], d, ll (at the final pi, d), n_iter, converged, b_in, N[V], hom, het (at the final pi, d),
 * ll_trace / d_trace [min(n_iter, trace_cap)]. */
int dmx_engine_get_prior_fit(dmx_engine*, double* pi, double* d, double* ll, int32_t* n_iter, int32_t* converged, int32_t* b_in, double* N,
                             double* hom, double* het, double* ll_trace, double* d_trace, int32_t trace_cap);
/* The records at (pi[V], d).  Results: dmx_engine_get_prior_calls(out[B]). */
int dmx_engine_prior_call(dmx_engine*, const dmx_prior_request*, const double* pi, double d);
int dmx_engine_get_prior_calls(dmx_engine*, dmx_prior_call* out);
int dmx_engine_prior_info(dmx_engine*, dmx_prior_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Goodness of fit of a call (no counterpart in the reference; later, still ABI 8).  Every other pass ranks
 * hypotheses against each other; this one asks whether a barcode's hypothesis explains its reads at all.  Barcode b carries ONE
 * hypothesis hyp[b] = (v1, v2) with alpha[b] and rho[b]: v1 = -1 = not used; v2 = -1 = a singlet of v1; otherwise a doublet of two
 * different samples, alpha the share of v2's reads; rho the fraction of reads from a soup of ALT frequencies a[n_snps].  Components c
 * and weights W_c are the existing profiles':
 *   singlet   c = g = 0, 1, 2:       W_c = gp[i][v1][g],                p_c = (1 - rho) g / 2 + rho a_i             (dmx_engine_ambient)
 *   doublet   c = (l, m), l-major:   W_c = gp[i][v1][l] gp[i][v2][m],   p_c = (1 - rho) (0.5 l + (m - l) 0.5 alpha) + rho a_i
 *             (float32 widened to float64: the product is exact)                                           (dmx_engine_ambient_doublet)
 * A pair (b, i) with n stored reads enters with its FIRST m = min(n, M) reads in stored order, M = max_reads in [1, 8]; stored order
 * does not depend on the alleles, so the sub-likelihood has a known law under the hypothesis.  For an allele pattern y in {0, 1}^m
 * (an integer; bit r = the allele of read r), with mat / err the phred tables at read r's base quality:
 *   t_r(c, 0) = mat (1 - p_c) + (err / 3) p_c,   t_r(c, 1) = (err / 3) (1 - p_c) + mat p_c     (two products, one sum; 1 - p_c rounded once)
 *   F_c(y)    = t_0(c, y_0) t_1(c, y_1) ... in stored order;   L(y) = sum_c W_c F_c(y) in component order.
 * Conditional on every read being stored, Pr(y) = L(y) / sum_y' L(y') (the per-read normaliser mat + err / 3 does not depend on c).
 * With x the observed pattern, c0 = log L(x) and u(y) = log L(y) - c0 (the log is dmx_log), over y ascending
 *   S0 = sum L(y),   S1 = sum L(y) u(y),   S2 = sum L(y) (u(y) u(y))       (a pattern with L(y) = 0 adds nothing to any of them),
 * and the pair adds   obs += c0,   mean += c0 + S1 / S0,   var += max(0, S2 / S0 - (S1 / S0)^2).
 * A pair with no stored read, or where a hypothesised sample's gp row is all zero, contributes nothing and is not counted.  A pair
 * with L(x) = 0, or whose S0 is 0 or not finite, contributes nothing either and is counted in n_zero[b].  n_snp[b] / n_read[b] count the
 * pairs / reads (m per pair) that contributed, n_trunc[b] those of them with n > M.  No rescaling is needed: the smallest non-zero
 * term is eight factors >= err(127) / 3 times a product of two float32 subnormals, still a normal float64.  Unused barcodes get zero
 * rows.  Without truncation obs[b] is dmx_engine_ambient's LL at (v1, rho), or dmx_engine_ambient_doublet's at (v1, v2, alpha, rho), up
 * to rounding.
 * Operations (binary64, every product, sum and quotient rounded on its own: no contraction; tests/contract_emul.cpp restates them and
 * tests/test_gpu_contract_bits.py compares the bits): om = 1 - rho, ra = rho a_i (rho = NULL: rho = 0 and ra = 0); c_g = 0.5 g for a singlet,
 * c_lm = 0.5 l + ((m - l) 0.5) alpha for a doublet (the product with alpha and the sum rounded); p_c = om c_c + ra; err / 3 rounded once;
 * F_c = t_0, then F_c = F_c t_r; L = W_0 F_0, then L = L + W_c F_c; S0, S1, S2 start at +0 and take L, L u and L (u u) (u u first);
 * e1 = S1 / S0 and d = S2 / S0 - e1 e1 with IEEE divisions, mean takes c0 + e1 (that sum first), var takes d when d > 0 and +0 otherwise.
 * L(y) != 0 is a positive normal number (below), so every log is dmx_log.
 * Summation plan: a barcode's pairs in stored order are dealt to 64 serial sums (pair k of the barcode goes to sum k mod 64, in
 * ascending k; k counts every pair of the barcode, whether it contributes or not; each sum starts at +0); the 64 sums are then added
 * serially onto +0, sum 0 first.  No floating-point atomics: b's seven outputs depend on b's own pairs
 * and reads, its hypothesis, M, and the gp rows and a entries it touches only — not on B, the other barcodes, what ran before, the
 * stream, or where hyp lives.  The call runs on the engine's stream, synchronises it before returning (host inputs may be freed then),
 * uses buffers of its own and leaves every other result of the engine as it was.
 * DMX_ERR_ARG: max_reads outside [1, 8]; an alpha or rho outside [0, 1] or not finite; an a_i outside [0, 1]; a hypothesis that is none
 * of unused (v1 = -1), a sample in [0, V) with v2 = -1, or two different samples in [0, V); rho without ambient; n_cells / n_snps that
 * do not match the staged pileup / the genotype matrix.  DMX_ERR_STATE: no pileup or no genotypes yet, or a query before a call.
 * DMX_ERR_NOMEM: the outputs do not fit the free device memory (earlier results stay readable). */
typedef struct {
  int32_t n_cells;             /* = the staged pileup's n_cells */
  int32_t n_snps;              /* = the genotype matrix's n_snps */
  int32_t hyp_memory;          /* DMX_MEM_HOST or DMX_MEM_DEVICE: where `hyp` lives */
  int32_t max_reads;           /* M, 1..8 */
  const int32_t* hyp;          /* [n_cells][2] */
  const double* alpha;         /* [n_cells] float64 in [0, 1], HOST (read for every barcode; used by doublets) */
  const double* rho;           /* [n_cells] float64 in [0, 1], HOST; NULL = 0 */
  const double* ambient;       /* [n_snps] float64 in [0, 1], HOST; NULL only when rho is NULL */
  int32_t reserved[4];         /* 0 */
} dmx_fit_request;
typedef struct {
  double  kernel_ms;           /* HIP-event time of the last call's k_fit launches (singlets, then doublets) */
  int64_t bytes;               /* device bytes of the call's buffers */
  int64_t n_trunc, n_zero;     /* totals over the barcodes */
  int32_t n_cells, n_used, n_singlet, n_doublet;
  int32_t max_reads;
  int32_t reserved[3];
} dmx_fit_info;
int dmx_engine_fit(dmx_engine*, const dmx_fit_request*);
/* Device->host copies of the last call's results (any pointer may be NULL): obs / mean / var [B] f64, n_snp / n_read / n_trunc /
 * n_zero [B] i32. */
int dmx_engine_get_fit(dmx_engine*, double* obs, double* mean, double* var, int32_t* n_snp, int32_t* n_read, int32_t* n_trunc,
                       int32_t* n_zero);
int dmx_engine_fit_info(dmx_engine*, dmx_fit_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Continuous mixing share of a doublet (no counterpart in the reference; later, still ABI 8).  Every pass that
 * names a doublet scores it at listed shares; these two calls treat the share alpha of v2's reads as a parameter.  The model is
 * dmx_engine_ambient_doublet's, with ONE contamination rho_b per barcode (rho = NULL: 0) instead of a grid, so the values compare with
 * dmx_engine_ambient / _ambient_doublet.  For barcode b, the pair (v1, v2), entries k = 3 l + m (l of v1, m of v2):
 *   p_lm = (1 - rho) (0.5 l + (m - l) 0.5 alpha) + rho a_i,   t_r,lm = pR_r (1 - p_lm) + pA_r p_lm,   f_lm = product over the reads of t_r,lm,
 *   L_i = sum_lm w_lm f_lm,  w_lm = gp[i][v1][l] gp[i][v2][m],   LL(alpha) = sum_i log L_i,
 * and its derivatives in alpha, with  s_lm = (1 - rho) 0.5 (m - l),  u_r,lm = (pA_r - pR_r) / t_r,lm,  S1_lm = sum_r u,  S2_lm = sum_r u u:
 *   f'_lm = f_lm s_lm S1_lm,   f''_lm = f_lm ((s_lm S1_lm)^2 - s_lm^2 S2_lm),   D1_i = L'_i / L_i,   D2_i = L''_i / L_i - D1_i^2,
 *   LL' = sum_i D1_i,   LL'' = sum_i D2_i.
 * The three entries l = m have s = 0: they add to L only.  As for dmx_engine_ambient_doublet, a pair with no stored read, or where
 * either sample's gp row is all zero, contributes nothing and is not counted.  With one-hot gp rows LL is concave in alpha; with soft
 * rows it need not be, and dmx_engine_share_fit finds a LOCAL maximum.
 * Operations (binary64, every product, sum and quotient rounded on its own: IEEE divisions, no contraction; tests/contract_emul.cpp restates
 * them and tests/test_gpu_contract_bits.py compares the bits), entries in the order k:
 *   p_lm      om = 1 - rho, ra = rho a_i;  c_lm = 0.5 l + ((m - l) 0.5) alpha;  p_lm = om c_lm + ra,  q_lm = 1 - p_lm;  s_lm = (om 0.5) (m - l).
 *             c_lm is this expression at every alpha, 0 and 1 included (no special case: at 0 it is 0.5 l, at 1 it is 0.5 l + (m - l) 0.5);
 *   read r    t = pR q_lm + pA p_lm;  f_lm = t of the first stored read, then f_lm t;  for l != m:  u = (pA - pR) / t,  S1 += u,  S2 += u u
 *             (from +0).  A factor t = 0 makes f_lm = 0 and takes u = 0: the entry then adds nothing to L, L' or L''.  After every eighth
 *             read an entry with 0 < f_lm < 2^-300 is rescaled into E_lm exactly as dmx_engine_ambient_doublet does (at every depth:
 *             below 8 reads E_lm stays 0);
 *   pair      E = max E_lm over the entries with w_lm != 0 and f_lm > 0;  T_lm = w_lm ldexp(f_lm, max(E_lm - E, -1100)) where w_lm != 0,
 *             else +0;  L = T_00, then L + T_lm;  over the six l != m in entry order  x = s_lm S1_lm,  y = x x - (s_lm s_lm) S2_lm,
 *             L' = T x of the first, then L' + T x;  L'' likewise with y;  lg = dmx_log(L), and when E != 0
 *             lg = fma(E, DMX_LOG_LN2HI, fma(E, DMX_LOG_LN2LO, lg));  D1 = L' / L;  D2 = L'' / L - D1 D1.  The scale 2^-E is common to L, L' and
 *             L'' and cancels in D1 and D2.  Without an entry to take E from, L = 0: lg = -inf and D1, D2 are NaN (0 / 0: that they are NaN
 *             is the contract, their sign and payload are not).
 *
 * dmx_engine_share_scan: for anchors[b][t] (t < T <= 4; -1 = slot not used) and EVERY partner v != anchor, v < V <= 1024, the three
 * numbers LL(0), LL'(0), LL''(0) of the pair (anchor, v) — the score statistic of "v is in the droplet too" is z = LL'(0) / sqrt(-LL''(0)).
 * At alpha = 0 p_lm does not depend on m, so the read loop runs for l = 0, 1, 2 once per pair for all partners (c_l = 0.5 l; E is the
 * maximum over the l with gp[i][anchor][l] != 0 and f_l > 0, which is the rule above for any partner whose row is not all zero;
 * F_l = ldexp(f_l, max(E_l - E, -1100)), +0 where gp[i][anchor][l] = 0 or f_l = 0; T_lm = w_lm F_l where w_lm != 0).  Each (b, t, v) is ONE
 * serial sum per output over b's pairs in stored (ascending SNP) order, starting at +0.  out[b][t][v] = (LL, LL', LL''); the row of
 * v = anchor and the rows of unused slots are zero.  n_snp / n_read [b][t] count the pairs / reads with a stored read and a non-zero
 * anchor row (a partner whose own row is all zero at a pair skips that pair): they are the anchor's counts, the same for every partner,
 * and n_read adds ALL stored reads of each such pair.  In the read loop u, S1 and S2 are kept for each l (every l has an m != l), and
 * the six l != m entries take x = s_lm S1_l, y = x x - (s_lm s_lm) S2_l.
 *
 * dmx_engine_share_fit: for candidates cand[b][c] = (v1, v2) (c < C <= 8; v1 = -1 = slot not used; otherwise two different samples) the
 * share alpha_hat in [0, 1] that maximises LL, by a safeguarded Newton iteration on the device; an "evaluation" gives LL, LL', LL'' at one
 * alpha:
 *    1. evaluate at 0 and at 1;
 *    2. if LL'(0) <= 0 and LL'(1) >= 0: alpha_hat = the end with the larger LL, 0 on a tie;
 *    3. else if LL'(0) <= 0: alpha_hat = 0;
 *    4. else if LL'(1) >= 0: alpha_hat = 1;
 *    5. otherwise lo = 0, hi = 1, alpha = start;
 *    6. evaluate at alpha;
 *    7. lo = alpha if LL' > 0, else hi = alpha;
 *    8. alpha' = alpha - LL' / LL'' when LL'' < 0 and lo < alpha' < hi, otherwise alpha' = (lo + hi) / 2;
 *    9. stop when |alpha' - alpha| <= tol, or when this was evaluation number max_iter of step 6 (DMX_SHARE_NOT_CONVERGED); otherwise
 *       alpha = alpha' and back to 6;
 *   10. one final evaluation at alpha_hat = alpha' (DMX_SHARE_INTERIOR).
 * In cases 2 to 4 the values at alpha_hat are those of step 1.  If a value of step 1 is not finite nothing is iterated: alpha_hat = 0
 * with DMX_SHARE_AT_0 | DMX_SHARE_NONFINITE.  DMX_SHARE_FLAT: LL''(alpha_hat) >= 0 (no standard error; a pair of samples with the same
 * one-hot rows gives LL' = LL'' = 0 and ends in case 2 at 0).  DMX_SHARE_NONFINITE: a value at 0, 1 or alpha_hat is not finite.  With
 * probe in [0, 1] one more evaluation at alpha = probe is returned (not counted in n_eval); probe < 0: none, zeros.  The probe is
 * evaluated whichever way the driver left, the non-finite exit of step 1 included, and does not enter the status.  n_snp / n_read are
 * those of the evaluation at 0 (they do not depend on alpha).
 * Summation plan of one evaluation: as dmx_engine_fit — pair k of the barcode (k counts every pair, contributing or not) goes to serial
 * sum k mod 64, each from +0 in ascending k; the 64 sums are added serially onto +0, sum 0 first; the same for LL, LL' and LL''.
 * values[b][c][13] = alpha_hat | LL, LL', LL'' at alpha_hat | at 0 | at 1 | at probe;  counts[b][c][4] = n_eval (steps 1, 6, 10), status,
 * n_snp, n_read.  Unused slots get zeros.
 *
 * Both calls: no floating-point atomics; a result's bits depend on b's data, the pair, rho_b, a, start / tol / max_iter / probe and V
 * only — not on B, T or C, the slot, where anchors / cand live, nrd_width, the other barcodes or what ran before.  They run on the
 * engine's stream, synchronise it before returning (host inputs may be freed then), use buffers of their own and leave every other result
 * of the engine as it was.
 * DMX_ERR_ARG: T outside [1, 4]; C outside [1, 8]; V > 1024 (scan); an id outside [-1, V); v1 = v2; a rho_b or a_i outside [0, 1] or not
 * finite; rho without ambient; tol <= 0; max_iter outside [1, 200]; start outside (0, 1); a probe above 1 or NaN; n_cells / n_snps that do
 * not match the staged pileup / the genotype matrix.  DMX_ERR_STATE: no pileup or no genotypes yet, or a query before a call.
 * DMX_ERR_NOMEM: the outputs do not fit the free device memory (checked before anything is allocated; earlier results stay readable). */
#define DMX_SHARE_INTERIOR      1
#define DMX_SHARE_AT_0          2
#define DMX_SHARE_AT_1          4
#define DMX_SHARE_NOT_CONVERGED 8
#define DMX_SHARE_FLAT          16
#define DMX_SHARE_NONFINITE     32
typedef struct {
  int32_t n_cells;             /* = the staged pileup's n_cells */
  int32_t n_snps;              /* = the genotype matrix's n_snps */
  int32_t n_anchor;            /* T, 1..4 */
  int32_t anchor_memory;       /* DMX_MEM_HOST or DMX_MEM_DEVICE: where `anchors` lives */
  const int32_t* anchors;      /* [n_cells][n_anchor] */
  const double* rho;           /* [n_cells] float64 in [0, 1], HOST; NULL = 0 */
  const double* ambient;       /* [n_snps] float64 in [0, 1], HOST; NULL only when rho is NULL */
  int32_t reserved[4];         /* 0 */
} dmx_share_scan_request;
typedef struct {
  int32_t n_cells;             /* = the staged pileup's n_cells */
  int32_t n_snps;              /* = the genotype matrix's n_snps */
  int32_t n_cand;              /* C, 1..8 */
  int32_t cand_memory;         /* DMX_MEM_HOST or DMX_MEM_DEVICE: where `cand` lives */
  const int32_t* cand;         /* [n_cells][n_cand][2] */
  const double* rho;           /* [n_cells] float64 in [0, 1], HOST; NULL = 0 */
  const double* ambient;       /* [n_snps] float64 in [0, 1], HOST; NULL only when rho is NULL */
  double  start;               /* in (0, 1); the front ends use 0.5 */
  double  tol;                 /* > 0; the front ends use 1e-6 */
  double  probe;               /* in [0, 1]: one more evaluation there; negative: none */
  int32_t max_iter;            /* 1..200; the front ends use 30 */
  int32_t reserved[5];         /* 0 */
} dmx_share_fit_request;
typedef struct {
  double  scan_ms, fit_ms;     /* HIP-event times of the last k_share_scan / k_share_fit */
  int64_t scan_bytes, fit_bytes;   /* device bytes of each call's buffers */
  int64_t scan_entries;        /* (b, t, v) entries scored: used anchor slots x (V - 1) */
  int64_t fit_used, fit_evals; /* candidate slots in use; evaluations run over them (the probe included) */
  int32_t n_cells, n_samples, n_anchor, n_cand;
  int32_t have_scan, have_fit; /* which of the two has run on the staged pileup */
  int32_t reserved[4];
} dmx_share_info;
int dmx_engine_share_scan(dmx_engine*, const dmx_share_scan_request*);
/* Device->host copies of the last scan (any pointer may be NULL): out[B][T][V][3] f64, n_snp_read[B][T][2] i32. */
int dmx_engine_get_share_scan(dmx_engine*, double* out, int32_t* n_snp_read);
int dmx_engine_share_fit(dmx_engine*, const dmx_share_fit_request*);
/* Device->host copies of the last fit (any pointer may be NULL): values[B][C][13] f64, counts[B][C][4] i32. */
int dmx_engine_get_share_fit(dmx_engine*, double* values, int32_t* counts);
int dmx_engine_share_info(dmx_engine*, dmx_share_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Site audit: goodness of fit per SNP (no counterpart in the reference; later, still ABI 8).  dmx_engine_fit asks
 * whether a barcode's call explains that barcode's reads, summed over its SNPs; this call asks the transposed question: does SNP i's row
 * of the genotype matrix explain the reads the pool holds there, summed over the barcodes?  The request's fields are dmx_fit_request's,
 * with the same meaning and the same checks (one hypothesis hyp[b] = (v1, v2), alpha[b], rho[b], ambient a[n_snps], M = max_reads).
 * Per-pair terms: exactly dmx_engine_fit's, operation for operation, as the block above states them — which pairs count (a stored read,
 * no all-zero gp row of a hypothesised sample), the first m = min(n, M) reads in stored order, W_c, p_c, t_r, F_c, L(y), c0 = log L(x),
 * S0, S1, S2 over y ascending, e1 = S1 / S0, d = S2 / S0 - e1 e1, and the rule for n_zero (L(x) = 0, or S0 zero or not finite: the pair
 * contributes nothing and is counted in n_zero).  Two more sums run over y ascending from +0, a pattern with L(y) = 0 adding nothing:
 * with k(y) the number of ALT reads in y (an exact small integer as a double),
 *   A1 += L(y) k(y),   A2 += L(y) (k(y) k(y))   (the product of the k's first),   a1 = A1 / S0,
 * the pair's signed ALT excess is k(x) - a1 and its variance max(0, A2 / S0 - a1 a1) (IEEE divisions, every operation rounded on its own).
 * Outputs per SNP i, summed over the counted pairs at i:
 *   obs += c0,  mean += c0 + e1,  var += max(0, d),  exc += k(x) - a1,  vexc += max(0, A2 / S0 - a1 a1)                   (float64)
 *   n_cell (pairs), n_read (m per pair), n_alt (k(x) per pair: observed ALT among the reads used), n_trunc (pairs with n > M), n_zero  (int32)
 * A SNP that no counted pair covers gets zero rows.  Z = (obs - mean) / sqrt(var) is the site's fit; exc / sqrt(vexc) tells
 * unexplained ALT reads (> 0) from missing ones (< 0).
 * (tests/contract_emul.cpp restates the terms and the plan below with dmx_engine_fit's own per-pair code; tests/test_gpu_contract_bits.py
 * compares the bits.)
 * Summation plan: the used barcodes are listed singlet hypotheses first, then doublet hypotheses, each in ascending cell id (the order
 * in which dmx_engine_fit lists them).  Each of the two lists is cut into chunks of 64 consecutive entries; the last chunk of a list may
 * be short and no chunk straddles the two lists.  For a SNP, the terms of a chunk's barcodes are added onto +0 in list order (a
 * barcode has at most one pair per SNP); the chunk partials are then added onto +0 in ascending chunk order.  Slab width, launch
 * geometry and the number of buffer waves are not part of the contract.  No floating-point atomics: a SNP's ten numbers depend only on
 * the pairs at that SNP, their barcodes' hypotheses and list positions, M, and the gp rows and a_i touched — not on the other SNPs,
 * partial_bytes, the stream, where hyp lives, or what ran before.  The call runs on the engine's stream, synchronises it before
 * returning, uses buffers of its own (and the refinement's slab table of the staged pileup, which it builds when the refinement has
 * not) and leaves every other result of the engine as it was.
 * partial_bytes: 0 = the default budget of the chunk-partial buffer (64 bytes per chunk and SNP), 4 GiB or a sixth of the free memory
 * as for dmx_engine_refine_genotypes; otherwise the cap on that buffer.  The chunks are processed in waves that fit it.
 * DMX_ERR_ARG: every case of dmx_engine_fit, and a partial_bytes that is negative or below one chunk's worth (64 n_snps).
 * DMX_ERR_STATE: no pileup or no genotypes yet, or a query before a call (dmx_engine_set_pileup clears the results).
 * DMX_ERR_NOMEM: the buffers do not fit the free device memory (earlier results stay readable). */
typedef struct {
  int32_t n_cells;             /* = the staged pileup's n_cells */
  int32_t n_snps;              /* = the genotype matrix's n_snps */
  int32_t hyp_memory;          /* DMX_MEM_HOST or DMX_MEM_DEVICE: where `hyp` lives */
  int32_t max_reads;           /* M, 1..8 */
  const int32_t* hyp;          /* [n_cells][2] */
  const double* alpha;         /* [n_cells] float64 in [0, 1], HOST */
  const double* rho;           /* [n_cells] float64 in [0, 1], HOST; NULL = 0 */
  const double* ambient;       /* [n_snps] float64 in [0, 1], HOST; NULL only when rho is NULL */
  int64_t partial_bytes;       /* cap on the chunk-partial buffer; 0 = default */
  int32_t reserved[4];         /* 0 */
} dmx_site_fit_request;
typedef struct {
  double  kernel_ms;           /* HIP-event time of the last call's k_site_partial / k_site_fold launches */
  int64_t bytes;               /* device bytes of the call's buffers, the partials included */
  int64_t partial_bytes;       /* ... of the chunk-partial buffer */
  int64_t n_trunc, n_zero;     /* totals over the SNPs */
  int32_t n_chunks, n_waves;   /* chunks of 64 barcodes; waves of chunks the partial buffer held in turn */
  int32_t chunk_cells, slab_snps;
  int32_t n_cells, n_snps, n_used, n_singlet, n_doublet;
  int32_t max_reads;
  int32_t reserved[4];
} dmx_site_fit_info;
int dmx_engine_site_fit(dmx_engine*, const dmx_site_fit_request*);
/* Device->host copies of the last call's results (any pointer may be NULL): obs / mean / var / exc / vexc [S] f64, n_cell / n_read /
 * n_alt / n_trunc / n_zero [S] i32. */
int dmx_engine_get_site_fit(dmx_engine*, double* obs, double* mean, double* var, double* exc, double* vexc, int32_t* n_cell,
                            int32_t* n_read, int32_t* n_alt, int32_t* n_trunc, int32_t* n_zero);
int dmx_engine_site_fit_info(dmx_engine*, dmx_site_fit_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Model-drawn null pool (no counterpart in the reference; later, still ABI 8).  The parametric bootstrap of the
 * staged pileup: its structure stays — which barcode covers which SNP, with how many reads, at which base qualities — and every stored
 * read's allele is drawn again from dmx_engine_fit's law under the barcode's hypothesis.  In the result the truth is known and the
 * model holds exactly, so what a statistic does there is its null law at this pool's depth.  The redrawn pileup has the source's exact
 * layout; only bit 7 (the allele) of a read byte changes, the base quality (the low 7 bits) is kept.
 * The law is dmx_engine_fit's: hyp[b] = (v1, v2) with alpha[b], rho[b] and the soup a[n_snps] mean what they mean in dmx_fit_request,
 * the components c, their weights W_c and ALT shares p_c are the ones stated there.  For a pair (b, i) with n >= 1 stored reads a
 * genotype is drawn for v1, and one for v2 if the hypothesis is a doublet — independently, each from its own gp row; W_c is the product
 * of the two rows' entries, so this IS the draw of the component.  Then EVERY stored read r = 0 .. n - 1 (not only the first M) gets a
 * new allele in stored order.  Pairs without stored reads (allele-2-only, see dmx_pileup) and unused barcodes (v1 = -1) are copied as
 * they are.
 * Bits (binary64, every product, sum and quotient rounded on its own: no contraction; integers mod 2^64; mix64 is dmx_engine_compose's;
 * GOLD = 0x9E3779B97F4A7C15; barcode b has the id = index_base + b; n_snp is the pair's SNP id):
 *   read uniform                    u  = mix64(mix64(seed + GOLD (4 id + 1)) + (n_snp << 32 | r)) >> 32
 *   genotype uniform, PAIR, slot s  ug = mix64(mix64(seed + GOLD (4 id + 2 + s)) + (n_snp << 32)) >> 32          (s = 0 for v1, 1 for v2)
 *   genotype uniform, DONOR, sample v   ug = mix64(mix64(geno_seed + GOLD (4 v + 2)) + (n_snp << 32)) >> 32
 *     DONOR depends on neither the barcode, the slot, seed nor index_base: every barcode of donor v, in every replicate, sees the same
 *     genotype at SNP i, as in a real pool.  PAIR draws a genotype per pair, which is dmx_engine_fit's own law.  The first-level keys of
 *     one barcode's read stream (4 id + 1) and its PAIR genotype streams (4 id + 2, 4 id + 3) are different multiples of GOLD.
 *   genotype from a row (w0, w1, w2), float32 widened:   c01 = w0 + w1,   s = c01 + w2,   x = ((double) ug 2^-32) s,
 *     g = 0 if x < w0, else 1 if x < c01, else 2.   A genotype of weight zero is never drawn: x >= 0 rules out g = 0 at w0 = 0; w1 = 0
 *     makes c01 = w0, an empty interval; and x < s strictly (ug 2^-32 <= 1 - 2^-32, s a normal number whose spacing is far finer), so
 *     with w2 = 0, where s = c01, g = 2 is never reached.
 *   a row that skips the pair: a hypothesised sample's row is all zero, or has a negative or non-finite entry.  The pair's reads are
 *     copied unchanged, its geno entries stay -1, and it is counted in n_pairs_skipped.
 *   read: om = 1 - rho, ra = rho a_i, c_c and p_c = om c_c + ra exactly as dmx_engine_fit states them, for the drawn component only
 *     (c_g = 0.5 g; c_lm = 0.5 l + ((m - l) 0.5) alpha); with mat / err the phred tables at the read's base quality, e3 = err / 3 rounded once:
 *       q1 = 1 - p_c,   num = e3 q1 + mat p_c,   den = mat + e3,   q = num / den,   thr = (uint64) (q 4294967296.0)   (truncation);
 *     the new allele is 1 iff (uint64) u < thr: q = 0 never draws ALT, q = 1 (thr = 2^32) always does.  If !(q >= 0 && q <= 1) the read
 *     keeps its stored allele and is counted in n_reads_kept.  q is t_r(c, 1) / (t_r(c, 0) + t_r(c, 1)) of dmx_engine_fit: the law of
 *     a read's allele given that the read is stored.
 * One kernel, k_redraw, after a device copy of the read array: plain vector stores, no floating-point atomics, nothing from another
 * barcode.  A barcode's bytes depend only on its own pairs, its hypothesis, its id, the seeds, and the gp rows and a_i it touches — not on
 * B, the dense or sparse layout, nrd_width, what ran before, or where hyp lives.  The call runs on the engine's stream, synchronises it
 * before returning (host inputs may be freed then), uses buffers of its own and leaves every other result of the engine as it was.
 * DMX_ERR_ARG: every argument case of dmx_engine_fit (max_reads apart: there is none); a genotype_draw that is neither constant;
 * index_base < 0.  DMX_ERR_STATE: no pileup or no genotypes yet; the staged pileup is this engine's own redrawn or composed pileup;
 * a query before a call (dmx_engine_set_pileup clears the result).  DMX_ERR_NOMEM: the outputs do not fit the free device memory. */
#define DMX_REDRAW_PAIR  0
#define DMX_REDRAW_DONOR 1
typedef struct {
  int32_t n_cells;             /* = the staged pileup's n_cells */
  int32_t n_snps;              /* = the genotype matrix's n_snps */
  int32_t hyp_memory;          /* DMX_MEM_HOST or DMX_MEM_DEVICE: where `hyp` lives */
  int32_t genotype_draw;       /* DMX_REDRAW_PAIR or DMX_REDRAW_DONOR */
  const int32_t* hyp;          /* [n_cells][2], dmx_fit_request's meaning; v1 = -1: the barcode's reads are copied unchanged */
  const double* alpha;         /* [n_cells] float64 in [0, 1], HOST */
  const double* rho;           /* [n_cells] float64 in [0, 1], HOST; NULL = 0 */
  const double* ambient;       /* [n_snps] float64 in [0, 1], HOST; NULL only when rho is NULL */
  uint64_t seed, geno_seed;
  int64_t  index_base;         /* >= 0: barcode b is hashed as id = index_base + b */
  int32_t  reserved[4];        /* 0 */
} dmx_redraw_request;
typedef struct {
  double  kernel_ms;           /* HIP-event time of the last call's k_redraw (the copy of the read array before it is not in it) */
  int64_t bytes_read, bytes_written;   /* algorithmic device bytes of k_redraw alone: the used barcodes' pair headers, the gp rows and read
                                          bytes of their pairs with stored reads, 44 bytes of parameters per barcode; the redrawn read bytes,
                                          two geno bytes per drawn pair, 16 bytes of counts per barcode */
  int64_t n_pairs_drawn;       /* pairs of used barcodes with a stored read and usable rows */
  int64_t n_pairs_skipped;     /* ... with a stored read and a row that skips the pair */
  int64_t n_reads_drawn;       /* reads of drawn pairs that got a new allele */
  int64_t n_reads_kept;        /* reads of drawn pairs whose q was not in [0, 1] */
  int32_t n_cells, n_used, n_singlet, n_doublet;
  int32_t genotype_draw;
  int32_t reserved[3];
} dmx_redraw_info;
int dmx_engine_redraw(dmx_engine*, const dmx_redraw_request*);
/* The redrawn pileup as a DMX_MEM_DEVICE view (rd_* NULL: the caller attaches host counters where a consumer needs them), for
 * dmx_engine_set_pileup of ANOTHER engine or dmx_job.pileup: the same n_*, cell_pair_off, cell_read_off, pair_snp (NULL if dense),
 * pair_nrd and nrd_width as the staged source — the source's own arrays — and new reads[] owned by the engine.  Valid until the next
 * redraw / set_pileup / destroy of this engine. */
int dmx_engine_redrawn_pileup(dmx_engine*, dmx_pileup* out);
/* Device->host copies (either pointer may be NULL): reads [the view's n_reads]; geno [the view's n_pairs][2] int8, the drawn genotypes
 * of v1 and v2 per pair, -1 = not drawn (no stored read, a skipped pair, an unused barcode, the second slot of a singlet). */
int dmx_engine_get_redrawn(dmx_engine*, uint8_t* reads, int8_t* geno);
int dmx_engine_redraw_info(dmx_engine*, dmx_redraw_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Joint genotype tables (no counterpart in the reference; later, still ABI 8).  Every other pass compares reads
 * with genotype columns; this one compares genotype columns with each other: for every pair (a, b) of columns of two gp-style matrices
 * ga[n_snps][n_a][3] and gb[n_snps][n_b][3] (float32: VCF transforms, refined rows, cluster rows) the weighted 4 x 4 joint table of
 * their rows over the SNPs.  Relatedness, cross-run matching and the expected separability of two donors are functions of it.
 * Row transform, per (SNP i, column v), binary64, every operation rounded on its own (no contraction):
 *   s = ((double) g0 + (double) g1) + (double) g2.  The row is valid (m = 1.0) when s is finite and > 0 and all three entries are >= 0
 *   (a NaN fails that).  For a valid row p_x = (double) g_x / s (IEEE division); otherwise m = p_0 = p_1 = p_2 = 0.0.
 *   The row's 4-vector is r = (p_0, p_1, p_2, m).
 * Weights: the A side carries the optional weight c[n_snps] (float64): wa_i[x] = c_i ra_i[x], one rounding.  weight = NULL means every
 * c_i = 1.0 and gives the bits of an explicit array of ones.  A non-finite or negative c_i is DMX_ERR_ARG.
 * Table T[a][b][x][y], x, y in 0..3:  acc = +0.0, then for i = 0 .. n_snps - 1 in ascending order  acc = fma(wa_i[a][x], rb_i[b][y], acc)
 * — one single chain of fused multiply-adds per entry; no slabs, no partial sums, no floating-point atomics.  An entry's bits depend on
 * n_snps, the two columns and c only: not on n_a, n_b, the tile shape, the launch geometry, what else is in the call or what ran
 * before.  All terms are >= 0: nothing cancels.  T[..][3][3] is the weight of the jointly valid SNPs, T[..][x][3] a's marginal over
 * them, T[..][3][y] b's, and T[..][0..2][0..2] the joint genotype table.  With gb = NULL the full n_a x n_a table is computed; the
 * weight sits on the A side, so T[a][b] and the transpose of T[b][a] need not have the same bits.
 * Two kernels (csrc/dmx_kin.hpp): k_kin_rows (the row transform into [S][V][4] float64 images, the invalid rows counted per column)
 * and k_kin_tile (the contraction).  The call needs no pileup, runs on the engine's stream and synchronises it before returning (host
 * inputs may be freed then), owns its buffers and leaves every other result of the engine as it was.  n_snps = 0 gives a table of zeros.
 * DMX_ERR_ARG: a null argument; n_a or n_b outside [1, 4096]; n_snps < 0; reserved != 0; a bad weight; gb = NULL with n_b != n_a; a
 * g_memory that is neither constant.  DMX_ERR_STATE: ga = NULL without a staged genotype matrix, or with one of another shape; a get
 * or info call before a compare.  DMX_ERR_NOMEM: the buffers do not fit the free device memory (the message names the sizes). */
#define DMX_KIN_MAX_COLUMNS 4096
typedef struct {
  int32_t n_snps, n_a, n_b;
  const float*  ga;            /* [n_snps][n_a][3]; NULL: the engine's staged matrix (n_snps / n_a must equal its S / V) */
  const float*  gb;            /* [n_snps][n_b][3]; NULL: B is A (n_b must equal n_a) */
  const double* weight;        /* [n_snps] or NULL */
  int32_t g_memory;            /* DMX_MEM_HOST | DMX_MEM_DEVICE, for ga, gb and weight together */
  int32_t reserved;            /* 0 */
} dmx_kin_request;
typedef struct {
  double  rows_ms, tile_ms;    /* HIP-event times of the last call's k_kin_rows launches (both sides) and of its k_kin_tile */
  int64_t flop;                /* 2 * 16 * n_a * n_b * n_snps */
  int64_t bytes;               /* algorithmic device bytes: both gp matrices and the weight read, both images written and read once,
                                  the table written */
  int64_t n_invalid_a, n_invalid_b;   /* invalid rows over all columns of each side */
  int32_t n_snps, n_a, n_b;
  int32_t tile_a, tile_b;      /* columns of A and of B per workgroup of k_kin_tile in the last call */
  int32_t chunk_snps;          /* SNPs staged per trip */
  int32_t reserved[2];
} dmx_kin_info;
int dmx_engine_geno_compare(dmx_engine*, const dmx_kin_request*);
/* Device->host copies of the last call's results (any pointer may be NULL): table [n_a][n_b][4][4] f64; n_valid_a [n_a] and n_valid_b
 * [n_b] i32, the valid rows of each column. */
int dmx_engine_get_geno_compare(dmx_engine*, double* table, int32_t* n_valid_a, int32_t* n_valid_b);
int dmx_engine_geno_compare_info(dmx_engine*, dmx_kin_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Block-resolved likelihoods (no counterpart in the reference; later, still ABI 8).  Every call is a sum of
 * per-SNP terms over the whole genome; this pass gives the same sums per genomic BLOCK: with block[i] in [0, G) the block of SNP i,
 * for every barcode b and block g
 *   col[b][g][j]   the part of llksAB[j][0][0] — the singlet column that .best / .sing2 print — from b's pairs in block g, every j < V;
 *   l00[b][g][n]   the part of llks00[n], every n < A;
 *   ext[b][g][s]   the part of llksAB[j][k][n] for the caller's entry extra[b][s] = (j, k, n), s < E; an unused slot (j = -1) is +0;
 *   n_snp[b][g]    b's stored pairs whose SNP lies in block g.
 * Arithmetic: a value is ONE serial sum from +0 over the barcode's stored pairs whose SNP lies in block g, in stored order, of the
 * STRICT grid's own term for that entry, operation for operation: phase 1 with the one maximum shared by all
 * alphas, the refined division, + 1e-6 and the renormalisation (cmd_cram_demuxlet.cpp:600-663), the nine-term l-major sum from 0.0
 * (:675-681), dmx_log2, one add.  The same terms whether the engine is DMX_MODE_STRICT or DMX_MODE_FAST.  No partial sums, no
 * floating-point atomics, no contraction.  Hence: with G = 1 every value is the entry of dmx_engine_run_doublet's STRICT grid, bit for
 * bit; and for any G, block g's values are the STRICT grid of an engine that holds only block g's pairs.
 * Determinism: a barcode's values depend on its own pairs, the rows it touches, the alpha grid and block[] at its own SNPs only —
 * not on B, the other barcodes, E, what ran before, the stream or where `extra` lives.  Blocks that a barcode does not cover are +0
 * with n_snp 0.
 * The call runs on the engine's stream and synchronises it before returning (block[] and extra[] may be freed then), uses buffers of
 * its own and leaves every other result of the engine readable and unchanged.
 * DMX_ERR_ARG: a null argument; n_blocks < 1; a block[] that decreases or leaves [0, G); n_extra outside [0, 8]; an extra entry
 * whose j is not -1 and whose (j, k, n) is outside [0, V) x [0, V) x [0, A); an extra_memory that is neither constant; reserved != 0;
 * n_cells / n_snps that do not match the staged pileup / the genotype matrix; more than 4094 samples or 64 alphas (the anchored search's limits); a
 * genotype matrix that k_check_geno did not pass (a row that is not finite, non-negative and somewhere above 1e-30): refused as the
 * anchored search refuses it, since this pass has no fix-up either.
 * DMX_ERR_STATE: no pileup or no genotypes yet; dmx_engine_get_block_llk / _block_llk_info before a call (or after a new pileup).
 * DMX_ERR_NOMEM: the B G (V + A + E) doubles do not fit the free device memory (checked before anything is allocated; earlier
 * results stay readable). */
#define DMX_BLOCK_MAX_EXTRA 8
typedef struct {
  int32_t n_cells, n_snps;     /* = the staged pileup's n_cells, the genotype matrix's n_snps */
  int32_t n_blocks;            /* G >= 1 */
  int32_t n_extra;             /* E, 0..8 */
  const int32_t* block;        /* [n_snps], HOST: non-decreasing, every value in [0, G); ids that no SNP has are allowed */
  const int32_t* extra;        /* [n_cells][E][3] = (j, k, n); j = -1: slot unused; j = k allowed.  NULL when E = 0 */
  int32_t extra_memory;        /* DMX_MEM_HOST or DMX_MEM_DEVICE: where `extra` lives */
  int32_t reserved[4];         /* 0 */
} dmx_block_llk_request;
typedef struct {
  double  kernel_ms;           /* HIP-event time of the last call's k_block_col */
  double  zero_ms;             /* ... of zeroing col, l00, ext and n_snp before it */
  int64_t result_bytes;        /* device bytes of col, l00, ext and n_snp */
  int64_t n_entries;           /* entries evaluated: B (V + A) + used extra slots */
  int32_t n_cells, n_samples, n_alpha, n_blocks, n_extra;
  int32_t reserved[3];
} dmx_block_llk_info;
int dmx_engine_block_llk(dmx_engine*, const dmx_block_llk_request*);
/* Device->host copies of the last result (any pointer may be NULL): col[B][G][V], l00[B][G][A], ext[B][G][E] f64, n_snp[B][G] i32. */
int dmx_engine_get_block_llk(dmx_engine*, double* col, double* l00, double* ext, int32_t* n_snp);
int dmx_engine_block_llk_info(dmx_engine*, dmx_block_llk_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * BGZF members inflated on the device (no counterpart in the reference; later, still ABI 8).  An inflater owns
 * two SLOTS, each with a stream and device buffers of its own, so that the host-to-device copy, the kernel (k_bgzf_inflate: one
 * wavefront per member) and the device-to-host copy of consecutive batches overlap: submit(slot 0), submit(slot 1), wait(slot 0),
 * submit(slot 0), wait(slot 1), ...  It is independent of any dmx_engine and leaves GPU_MAX_HW_QUEUES alone.
 * Contract.  Member i is a raw DEFLATE stream (RFC 1951) of in_len[i] bytes at in + in_off[i], to be inflated into out_len[i]
 * bytes at out + out_off[i].  in_off[i] is a multiple of 4 and the host buffer is readable for in_len[i] + 8 bytes, rounded up to
 * a multiple of 4, from there (the scanner leaves 8 zero bytes after every member; what those bytes hold never matters: the decoder reads
 * bytes at or past in_len as zero).  The members' padded inputs must lie within max_in_bytes of one another and their outputs within
 * max_out_bytes; output ranges must not overlap.
 *   status[i] == 0  the stream's final block ended exactly at out_len[i] bytes, no more than in_len[i] bytes were consumed, and the
 *                   bytes are the ones zlib's inflate gives;
 *   status[i] != 0  refused (the value says why, see dmx_inflate_core.hpp): the member's output bytes are unspecified, but nothing
 *                   outside out + [out_off[i], out_off[i] + out_len[i]) was written.
 * out_len[i] == 0 is legal (the BGZF end-of-file member) and writes nothing.  A member with out_len > 65 536 or in_len > 65 536 + 64
 * is refused (a status, not an error) and none of its bytes are touched.  A member's status and bytes do not depend on n, on the
 * other members, on its position or on the slot.  No checksum is computed: CRC-32 is the caller's, over the bytes after the copy.
 * The device-to-host copies land at `out` itself (one copy per run of members whose ranges follow one another), so `in`, `out`
 * and the offset arrays must stay valid, and `out` untouched, until dmx_inflater_wait returns; page-locked buffers
 * (dmx_inflater_pin) let the copies run beside the host's work, pageable ones are correct but serialise.
 * Errors: DMX_ERR_NOGPU without a usable gfx950 device; DMX_ERR_ARG for a null argument, a slot that is not 0 or 1, n outside
 * [0, max_members], a negative or misaligned offset, spans above the inflater's sizes; DMX_ERR_STATE for a submit into a slot in
 * flight or a wait on an idle one; DMX_ERR_NOMEM when the buffers do not fit; DMX_ERR_HIP.  A submit that fails after it has queued
 * work synchronises the slot's stream before it returns: the caller's buffers are its own again and the slot is idle. */
typedef struct dmx_inflater dmx_inflater;
typedef struct {
  double  kernel_ms;           /* HIP-event time of the batch's k_bgzf_inflate */
  double  h2d_ms, d2h_ms;      /* ... of its host-to-device and device-to-host copies */
  int64_t h2d_bytes, d2h_bytes;
  int32_t n_members, n_accepted, n_refused;
  int32_t reserved[3];
} dmx_inflater_info;
int dmx_inflater_create(int32_t device, int32_t max_members, int64_t max_in_bytes, int64_t max_out_bytes, dmx_inflater** out);
int dmx_inflater_free(dmx_inflater*);
int dmx_inflater_submit(dmx_inflater*, int32_t slot, int32_t n, const uint8_t* in, const int64_t* in_off, const int32_t* in_len,
                        uint8_t* out, const int64_t* out_off, const int32_t* out_len);
/* Blocks until the slot's batch is done; status[n] of that batch; info may be NULL. */
int dmx_inflater_wait(dmx_inflater*, int32_t slot, int32_t* status, dmx_inflater_info* info);
/* submit into slot 0 + wait */
int dmx_inflater_run(dmx_inflater*, int32_t n, const uint8_t* in, const int64_t* in_off, const int32_t* in_len,
                     uint8_t* out, const int64_t* out_off, const int32_t* out_len, int32_t* status, dmx_inflater_info* info);
/* Page-locks / releases a host buffer of the caller's (hipHostRegister / hipHostUnregister); unpin before the memory is freed. */
int dmx_inflater_pin(void* ptr, int64_t bytes);
int dmx_inflater_unpin(void* ptr);

#ifdef __cplusplus
}
#endif
#endif
