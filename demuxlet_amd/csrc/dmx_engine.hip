// Device half of libdmx: the likelihood engine for one MI355X (gfx950).  Hand-written HIP, FP64 VALU + LDS; no MFMA
// (contraction lengths are 3 and 9), no library kernels.  Built with -ffp-contract=off: in STRICT mode every
// expression the reference evaluates is evaluated with the same operations in the same order (separate IEEE mul/add/
// div); the only fused operations are inside dmx_log(), our own replacement for libm's log().
//
//   k_gp0        a4  gp0s[s][l] = (sum_j g[s][j][l]) / V                       cmd_cram_demuxlet.cpp:390-401
//   k_singlet    a5  llks[c][k] += log(GL . g[s][k]),  llk0s[c] += log(GL . gp0s[s])        :412-461
//   k_doublet_*  a8+a9  pG[A][3][3] per covered pair, llksAB[c][j][k][n] += log(sum_lm g_j[l] g_k[m] pG[n][l][m]),
//                    llks00[c][n] likewise with gp0s                                        :576-710
//   k_reduce     a10,a11,a13  per-cell max / posterior sums / top-2 singlets / best doublet :713-734,:746-758,:799-828
//
// Order guarantee (what makes STRICT strict): every accumulator is owned by exactly one lane, which adds that cell's
// per-SNP terms in ascending SNP order — the order of the reference's std::map walks.  Terms themselves are computed
// by whichever lane is free (k_singlet stages them through LDS), which does not change any rounding.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <mutex>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <new>
#include <memory>
#include <functional>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <cxxabi.h>
#include <string>
#include <numeric>
#include <vector>

#include "dmx_internal.hpp"
extern char** environ;
#include "dmx_log.hpp"
#include "dmx_engine_state.hpp"
#include "dmx_hyp_plan.hpp"

using dmx::set_error;
using dmx::DevBuf; using dmx::Event; using dmx::EventPair; using dmx::Stream; using dmx::PinnedBuf;

namespace {

struct PileupView {
  int32_t B, S;
  int64_t R;                   // total read bytes
  const int64_t* cell_pair_off;
  const int64_t* cell_read_off;
  const int32_t* pair_snp;     // nullptr = dense
  const void* pair_nrd;
  const uint8_t* reads;
};

// Ordering of LDS stores and loads between the lanes of ONE wavefront: the LDS executes a wavefront's instructions in
// program order, so only the compiler has to be kept from moving them across this point.
#ifdef DMX_FENCE_VARIANT
#define DMX_WAVE_LDS_ORDER() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
#else
#define DMX_WAVE_LDS_ORDER() do { asm volatile("" ::: "memory"); __builtin_amdgcn_wave_barrier(); } while (0)
#endif

#ifndef DMX_ABLATE
#define DMX_ABLATE 0
#endif

constexpr int kThreads = 256;
constexpr int kLut = 3 * 128;   // mat | err/3 | 0.5-err/3
constexpr int kTab = kLut + DMX_LOG_TABLE_DOUBLES;   // device table buffer: read LUT, then dmx_log's {invc,logc} table
constexpr int kFirst = 256 * 3, kFinal = 257 * 3;     // then the singlet first-read tables (dmx::SingletTables)
constexpr int kTabK1 = kTab + kFirst + kFinal;
constexpr int kPair = 128 * 128 * 4;                    // then dmx::PairTables: second[16384][4] | final2[16384][4] (global memory only)
constexpr int kTriple = dmx::kTripleCodes * dmx::kTripleCodes * dmx::kTripleCodes * 4;   // then dmx::TripleTables: third | final3
constexpr int kTabAll = kTabK1 + 2 * kPair + 2 * kTriple;
constexpr int kTabLogLo = kTabAll;                      // then dmx_log_dd's second-order table (128 doubles)
constexpr int kTabLog2 = kTabAll + 128;                 // then dmx_log2's 256-bin {invc, logc} table (the doublet kernels' log, round 4)
constexpr int kTabLog32 = kTabLog2 + DMX_LOG2_TABLE_DOUBLES;   // then dmx_log2_lite32's split 32-bin table rc[32] | logc[32] (FAST k_doublet_sym, round 6)
constexpr int kTabTotal = kTabLog32 + DMX_LOG32_TABLE_DOUBLES;
// canonical-class log table (k_build_canon_logs): entries in the order of the final GL tables — one read (257, the last = no read) | two | three
constexpr int64_t kCanL2 = 257, kCanL3 = 257 + 128 * 128, kCanN = kCanL3 + (int64_t)dmx::kTripleCodes * dmx::kTripleCodes * dmx::kTripleCodes;
constexpr int kLut2 = 2 * 128;                           // the doublet kernels read mat | err/3 only (the third LUT part is the singlet kernels')
constexpr int kTab2 = kLut2 + DMX_LOG2_TABLE_DOUBLES;   // a doublet kernel's LDS table: read LUT (2 KB) | dmx_log2 table (4 KB) = 1 KB more than
                                                        // rounds 1-3's 3 + 2 KB: k_doublet_a2<64,4> keeps its three workgroups per CU (3 x 53.4 KB)
// stage a doublet kernel's tables: the read LUT from the head of the device buffer, dmx_log2's table from its tail
__device__ __forceinline__ void stage_k2_tables(double* s_tab, const double* __restrict__ tabs, int t, int nthreads) {
  for (int i = t; i < kLut2; i += nthreads) s_tab[i] = tabs[i];
  for (int i = t; i < DMX_LOG2_TABLE_DOUBLES; i += nthreads) s_tab[kLut2 + i] = tabs[kTabLog2 + i];
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ void k_gp0(const float* __restrict__ g, int32_t S, int32_t V, double* __restrict__ gp0) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)S * 3) return;
  const int64_t s = i / 3;
  const int l = (int)(i % 3);
  const float* row = g + (size_t)s * V * 3 + l;
  double acc = 0.0;                                   // calloc'ed, :391
  for (int32_t j = 0; j < V; ++j) acc += (double)row[(size_t)j * 3];   // :393-397 sequential over samples
  gp0[i] = acc / (double)V;                           // :398-400
}

// ---------------------------------------------------------------------------------------------------------------------
// IEEE-754 binary64 division with the reciprocal refinement shared between several numerators of one denominator.
// This is, operation for operation, the sequence the compiler emits for `a / b` (v_rcp_f64, two Newton steps, quotient,
// residual, correction) minus v_div_scale / v_div_fmas-scaling / v_div_fixup, which only act when an exponent is
// extreme; callers guarantee 2^-700 < a,b < 2^700 (otherwise they use the plain `/`).  Correctly rounded, so
// bit-identical to the reference's x86 divsd (checked on the device by dmx_debug_device_div).
__device__ __forceinline__ double rcp_refined(double b) {
  double y = __builtin_amdgcn_rcp(b);
  double e = __builtin_fma(-b, y, 1.0);
  y = __builtin_fma(y, e, y);
  e = __builtin_fma(-b, y, 1.0);
  y = __builtin_fma(y, e, y);
  return y;
}
__device__ __forceinline__ double div_by(double a, double b, double y) {
  const double q = a * y;
  const double r = __builtin_fma(-b, q, a);
  return __builtin_fma(r, y, q);
}

// The plain IEEE division for the (rare) deep pairs, kept out of line: inlined five or nine times it is the register-pressure
// peak of the FAST kernels, whose accumulators have to stay in registers across it.
__device__ __attribute__((noinline)) double div_slow(double a, double b) { return a / b; }

constexpr int kPark = 12;              // doubles of parked k_certify state per barcode: 4 chains | 4 event words | clean[2] | ok | pad
constexpr int kA2MaxV = 1024;            // widest soft-field panel of k_doublet_a2<256,16> (LDS: 32 / 16 / 8 genotype rows of V * 12 bytes + 12 KB)
constexpr int kAnMaxV4 = 368, kAnMaxV8 = 344;   // k_doublet_an's widest panels (its pG block is 9 / 18 KB instead of 4.5): 160 KB of LDS in all
constexpr uint32_t kSafeReads = 15;   // each read scales a likelihood by >= err(127)/3 > 2^-44: 15 reads stay above 2^-700

// ---- genotype likelihoods of a (cell, SNP) pair (cmd_cram_demuxlet.cpp:427-452) -----------------------------------------
// They start from a table entry chosen by the pair's read count and leading read bytes (dmx::SingletTables / PairTables /
// TripleTables, host-computed with the reference's IEEE operations): the whole answer for 0-3 reads, the state after
// three (two, one) reads for deeper pairs, whose loop then starts at read r0.  All tables live in one buffer (`tabs`), so
// a 32-bit element offset selects the entry.  The K1 kernels issue this gather a whole tile ahead of its use.
struct GlSeed { double g0, g1, g2; uint32_t r0; };     // r0: first read the loop still has to apply (>= n: none)
__device__ __forceinline__ GlSeed gl_seed(const double* __restrict__ tabs, uint32_t n, uint32_t rd4) {
  constexpr uint32_t oFirst = kTab, oFinal1 = kTab + kFirst, oSecond = kTabK1, oFinal2 = kTabK1 + kPair,
                     oThird = kTabK1 + 2 * kPair, oFinal3 = kTabK1 + 2 * kPair + kTriple;
  const uint32_t b0 = rd4 & 0xFFu, b1 = (rd4 >> 8) & 0xFFu, b2 = (rd4 >> 16) & 0xFFu;
  const uint32_t q0 = b0 & 127u, q1 = b1 & 127u, q2 = b2 & 127u;
  const bool two = n >= 2 && ((b0 | b1) & 0x40u) == 0;                          // both base qualities < 64: PairTables
  const bool three = n >= 3 && max(max(q0, q1), q2) < (uint32_t)dmx::kTripleBq;  // all three < 48: TripleTables
  const uint32_t i2 = ((((b0 & 0x80u) >> 1) | (b0 & 0x3Fu)) << 7) | (((b1 & 0x80u) >> 1) | (b1 & 0x3Fu));
  const uint32_t c0 = ((b0 & 0x80u) ? (uint32_t)dmx::kTripleBq : 0u) + q0, c1 = ((b1 & 0x80u) ? (uint32_t)dmx::kTripleBq : 0u) + q1,
                 c2 = ((b2 & 0x80u) ? (uint32_t)dmx::kTripleBq : 0u) + q2;
  const uint32_t i3 = __umul24(__umul24(c0, (uint32_t)dmx::kTripleCodes) + c1, (uint32_t)dmx::kTripleCodes) + c2;   // full-rate multiplies
  uint32_t off = oFirst + 3u * b0;
  off = two ? (n == 2 ? oFinal2 : oSecond) + 4u * i2 : off;
  off = three ? (n == 3 ? oFinal3 : oThird) + 4u * i3 : off;
  off = n == 1 ? oFinal1 + 3u * b0 : off;
  off = n == 0 ? oFinal1 + 3u * 256u : off;
  const double* p = tabs + off;
  GlSeed sd;
  sd.g0 = p[0]; sd.g1 = p[1]; sd.g2 = p[2];
  sd.r0 = n < 2 ? n : (three ? 3u : (two ? 2u : 1u));
  return sd;
}
// reads beyond a table's state (g0, g1, g2 after the pair's first r0 reads): continue the reference's loop from read r0, then the +1e-6 renormalisation
__device__ __forceinline__ void gl_continue(uint32_t r0, uint32_t n, uint32_t rd4, const uint8_t* __restrict__ reads, int64_t off,
                                            const double* __restrict__ lut, double& g0, double& g1, double& g2) {
  const bool safe = n <= kSafeReads;
  for (uint32_t r = r0; r < n; ++r) {
    const uint32_t byte = (r < 4) ? ((rd4 >> (8 * r)) & 0xFFu) : (uint32_t)reads[off + r];
    const uint32_t bq = byte & 127u;
    const bool alt = (byte >> 7) != 0;
    const double m = lut[bq], e3 = lut[128 + bq], h = lut[256 + bq];
    g0 *= alt ? e3 : m;                                                      // :437
    g1 *= h;                                                                 // :438
    g2 *= alt ? m : e3;                                                      // :439
    const double tmp = g0 + g1 + g2;                                         // :440
    if (safe) {
      const double y = rcp_refined(tmp);
      g0 = div_by(g0, tmp, y); g1 = div_by(g1, tmp, y); g2 = div_by(g2, tmp, y);   // :441-443
    } else {
      g0 /= tmp; g1 /= tmp; g2 /= tmp;
    }
  }
  g0 += 1e-6; g1 += 1e-6; g2 += 1e-6;                                        // :446-448
  const double tmp = g0 + g1 + g2;
  const double y = rcp_refined(tmp);
  g0 = div_by(g0, tmp, y); g1 = div_by(g1, tmp, y); g2 = div_by(g2, tmp, y);         // :449-452
}
__device__ __forceinline__ void gl_finish(const GlSeed& sd, uint32_t n, uint32_t rd4, const uint8_t* __restrict__ reads, int64_t off,
                                          const double* __restrict__ lut, double& G0, double& G1, double& G2) {
  G0 = sd.g0; G1 = sd.g1; G2 = sd.g2;
  if (sd.r0 < n) gl_continue(sd.r0, n, rd4, reads, off, lut, G0, G1, G2);
}


// the three singlet genotype likelihoods of one covered pair (:427-452): per read multiply, then renormalise to sum 1
__device__ __forceinline__ void pair_gl(const uint8_t* __restrict__ rd, uint32_t n, const double* s_lut, double& G0,
                                        double& G1, double& G2) {
  G0 = 1.0; G1 = 1.0; G2 = 1.0;                                            // :427
  const bool safe = n <= kSafeReads;
  for (uint32_t r = 0; r < n; ++r) {
    const uint32_t byte = rd[r];
    const uint32_t bq = byte & 127u;
    const bool alt = (byte >> 7) != 0;
    const double m = s_lut[bq], e3 = s_lut[128 + bq], h = s_lut[256 + bq];
    G0 *= alt ? e3 : m;                                                    // :437
    G1 *= h;                                                               // :438
    G2 *= alt ? m : e3;                                                    // :439
    const double tmp = G0 + G1 + G2;                                       // :440
    if (safe) {
      const double y = rcp_refined(tmp);
      G0 = div_by(G0, tmp, y); G1 = div_by(G1, tmp, y); G2 = div_by(G2, tmp, y);   // :441-443
    } else {
      G0 /= tmp; G1 /= tmp; G2 /= tmp;
    }
  }
  G0 += 1e-6; G1 += 1e-6; G2 += 1e-6;                                      // :446-448
  const double tmp = G0 + G1 + G2;
  const double y = rcp_refined(tmp);                                       // numerators >= 1e-6, tmp ~ 1
  G0 = div_by(G0, tmp, y); G1 = div_by(G1, tmp, y); G2 = div_by(G2, tmp, y);       // :449-452
}

// Inclusive prefix sum of v over segments of T consecutive lanes (T = 16, 32 or 64), on the VALU's DPP data path:
// four row-shift adds give the scan inside each 16-lane row, row_bcast:15 / row_bcast:31 carry the row totals.
template <int T>
__device__ __forceinline__ uint32_t seg_scan_incl(uint32_t v) {
  static_assert(T == 8 || T == 16 || T == 32 || T == 64, "segment width (8: the segment must start a 16-lane row)");
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1 (0 past the row start)
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
  if (T >= 16) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8
  if (T >= 32) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1,3
  if (T >= 64) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2,3
  return v;
}
// value of the last lane of this lane's T-wide segment
template <int T>
__device__ __forceinline__ uint32_t seg_last(uint32_t v, int lane) {
  if (T == 64) return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
  if (T == 32) {
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 31), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
    return lane < 32 ? a : b;
  }
  return (uint32_t)__shfl((int)v, T - 1, T);
}

// The first four stored read bytes of a pair as one (unaligned) 32-bit load; bytes past the pair's reads are never interpreted.
__device__ __forceinline__ uint32_t load_rd4(const PileupView& pv, int64_t off, uint32_t cnt) {
  uint32_t rd4 = 0;
  if (cnt > 0) {
    if (off + 4 <= pv.R) __builtin_memcpy(&rd4, pv.reads + off, 4);
    else for (int64_t i = off; i < pv.R; ++i) rd4 |= (uint32_t)pv.reads[i] << (8 * (int)(i - off));
  }
  return rd4;
}

// The value of the neighbouring lane (lane ^ 1: the other alpha of the same pair in phase 1) by DPP quad permutation [1,0,3,2] —
// two VALU moves instead of the two LDS-crossbar operations (ds_bpermute) that __shfl_xor becomes, in the middle of phase 1's
// dependent chain (products -> maximum -> neighbour's maximum -> reciprocal -> quotients).
// Both lanes of an (even, odd) pair get the ODD lane's value (quad permutation [1,1,3,3]): one DPP move per word, no select.
__device__ __forceinline__ double shfl_odd(double x) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), 0xF5, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), 0xF5, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shfl_xor1(double x) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), 0xB1, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), 0xB1, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// One 8-byte LDS read that the compiler must not pair with a neighbour: ds_read2_b64 is serviced as two 4 x 16-lane accesses
// (8 LDS cycles, 128 B/clk, MI355X_MICROARCH.md "LDS") where two ds_read_b64 take 2 + 2 — and the hot loops of the FAST doublet
// kernels read three doubles 8*VUS bytes apart per evaluation, which the load/store optimiser merges whenever it can.
__device__ __forceinline__ double lds_read_f64(const double* p) {
  return *(const volatile __attribute__((address_space(3))) double*)(const __attribute__((address_space(3))) double*)p;
}
// base + byte BYTE of w in ONE VALU instruction (SDWA operand select; the compiler emits v_bfe_u32 + v_add for the same expression)
template <int BYTE> __device__ __forceinline__ uint32_t add_byte_of(uint32_t base, uint32_t w) {
  uint32_t r;
  if constexpr (BYTE == 0) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(base), "v"(w));
  else if constexpr (BYTE == 1) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "v"(base), "v"(w));
  else if constexpr (BYTE == 2) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "v"(base), "v"(w));
  else asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(r) : "v"(base), "v"(w));
  return r;
}

// base + 16-bit half HALF of w, likewise (SDWA word select)
template <int HALF> __device__ __forceinline__ uint32_t add_word_of(uint32_t base, uint32_t w) {
  uint32_t r;
  if constexpr (HALF == 0) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(r) : "v"(base), "v"(w));
  else asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(r) : "v"(base), "v"(w));
  return r;
}
#ifndef DMX_FAST_PRODUCT
#define DMX_FAST_PRODUCT 0                        // 1: FAST k_doublet_sym takes ONE log per entry and full sub-tile, of the product of its terms — an experiment
                                                  // build only: cfg3 FAST K2 217 -> 159 ms, but the sums then round differently from the
                                                  // reference's own sequence of adds and sit up to 1.3e-9 from it at cfg3's depth (rms 2.6e-10; a log per term: 4e-11)
#endif
#ifndef DMX_SYM_ABLATIONS
#define DMX_SYM_ABLATIONS 0                       // 1: k_doublet_sym carries its timing-ablation switches (results WRONG) — experiment builds only
#endif
#ifndef DMX_SYM_NB
#define DMX_SYM_NB 3                              // entries per step of k_doublet_sym's software-pipelined phase 2 (0: off)
#endif
#ifndef DMX_SYM_TIMING
#define DMX_SYM_TIMING 0                          // timing builds only (results WRONG): 1 = phase-2 polynomial one FMA shorter, 2 = k ln 2 from an LDS look-up and one add
#endif                                            //   instead of cvt + fma, 3 = both — what a 2 048-bin table / a k-indexed table would buy
#ifndef DMX_SYM_HYB
#define DMX_SYM_HYB 0                             // k_doublet_sym's mix of the two FAST logs: 0 none, 1 every third entry of a lane through dmx_log2_lite32, 2 two of three, 3 all, 4 every second
#endif
#ifndef DMX_FAST_LITE_LOG
#define DMX_FAST_LITE_LOG 1                       // FAST phase-2 terms through dmx_log2_lite (6 FP64 instructions; csrc/dmx_log.hpp) — 0: dmx_log2 (10), as rounds 2-4
#endif
// the log of FAST mode's phase-2 terms (k_doublet_sym / _a2f / _anf)
__device__ __forceinline__ double dmx_log2_fastmode(double x, const double* __restrict__ T, const DmxLogPins& K) {
  return DMX_FAST_LITE_LOG ? dmx_log2_lite(x, T, K) : dmx_log2_fast_pinned(x, T, K);
}
#ifndef DMX_LDS_NOMERGE
#define DMX_LDS_NOMERGE 1                         // cfg3 FAST K2 309 -> 291 ms (0 restores the merged reads: kernel experiments only)
#endif

__device__ __forceinline__ uint32_t load_nrd(const void* __restrict__ base, int64_t p, int width) {
  if (width == 1) return ((const uint8_t*)base)[p];
  if (width == 2) return ((const uint16_t*)base)[p];
  return ((const uint32_t*)base)[p];
}

// Cells whose fast kernels met a log() argument outside the normal positive range: one byte per cell, and in front of the array
// (kFlagHead bytes) a word that says whether ANY cell of the launch was flagged — what the fix-up pass looks at first.
constexpr int kFlagHead = 16;
__device__ __forceinline__ void flag_cell(uint8_t* __restrict__ flagged, int32_t cell) { flagged[cell] = 1; *(flagged - kFlagHead) = 1; }
__device__ __forceinline__ bool flags_any(const uint8_t* __restrict__ flagged) { return *(const volatile uint8_t*)(flagged - kFlagHead) != 0; }

// Round 6: FINAL phase-1 values of the default grid {0, 0.5} — the five distinct alpha = 0.5 values q[l + m] and the three of alpha = 0 after the read loop AND
// the +1e-6 renormalisation of :649-663 (k_doublet_sym's phase 1, certify_pair_values<5>) —
// for every pair whose reads index a table: no read, one read, two reads of base quality < 64, three of base quality < 48 (K1's TripleTables codes).  One
// thread per entry runs the loop of :597-639 and the finish for BOTH alpha lanes (the maxima run across them): the operations of k_certify's two lanes on
// the same operands, hence the same bits.  A tile none of whose pairs is deeper takes its values from here and skips the seeds, the loop, the finish and
// the hand-over between the lanes (at 1.25 reads per pair: 93 % of the tiles; 43 % with the one- and two-read entries alone).
constexpr int kCFinStride = 8;                   // doubles per entry: alpha 0.5's five values, alpha 0's three (one 64-byte line)
constexpr int64_t kCFin1 = 1, kCFin2 = 1 + 256, kCFin3 = kCFin2 + 128 * 128,
                  kCFinN = kCFin3 + (int64_t)dmx::kTripleCodes * dmx::kTripleCodes * dmx::kTripleCodes;
__device__ __forceinline__ int32_t certify_final_index(uint32_t cnt, uint32_t rd4) {     // -1: the pair's reads are not in the table
  const uint32_t b0 = rd4 & 0xFFu, b1 = (rd4 >> 8) & 0xFFu, b2 = (rd4 >> 16) & 0xFFu;
  const uint32_t q0 = b0 & 127u, q1 = b1 & 127u, q2 = b2 & 127u;
  const uint32_t i2 = ((((b0 & 0x80u) >> 1) | (b0 & 0x3Fu)) << 7) | (((b1 & 0x80u) >> 1) | (b1 & 0x3Fu));
  const uint32_t c0 = ((b0 & 0x80u) ? (uint32_t)dmx::kTripleBq : 0u) + q0, c1 = ((b1 & 0x80u) ? (uint32_t)dmx::kTripleBq : 0u) + q1,
                 c2 = ((b2 & 0x80u) ? (uint32_t)dmx::kTripleBq : 0u) + q2;
  const uint32_t i3 = __umul24(__umul24(c0, (uint32_t)dmx::kTripleCodes) + c1, (uint32_t)dmx::kTripleCodes) + c2;
  int32_t idx = -1;
  idx = (cnt == 3 && max(max(q0, q1), q2) < (uint32_t)dmx::kTripleBq) ? (int32_t)kCFin3 + (int32_t)i3 : idx;
  idx = (cnt == 2 && ((b0 | b1) & 0x40u) == 0) ? (int32_t)kCFin2 + (int32_t)i2 : idx;
  idx = cnt == 1 ? (int32_t)kCFin1 + (int32_t)b0 : idx;
  idx = cnt == 0 ? 0 : idx;
  return idx;
}
__global__ void k_build_certify_finals(const double* __restrict__ tabs, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= kCFinN) return;
  uint32_t bytes[3] = {0u, 0u, 0u}; int nb;
  if (e < kCFin1) nb = 0;
  else if (e < kCFin2) { bytes[0] = (uint32_t)(e - kCFin1); nb = 1; }
  else if (e < kCFin3) {
    const uint32_t i2 = (uint32_t)(e - kCFin2), c0 = i2 >> 7, c1 = i2 & 127u;
    bytes[0] = ((c0 & 0x40u) << 1) | (c0 & 0x3Fu); bytes[1] = ((c1 & 0x40u) << 1) | (c1 & 0x3Fu); nb = 2;
  } else {
    uint32_t c = (uint32_t)(e - kCFin3);
    const uint32_t c2 = c % (uint32_t)dmx::kTripleCodes; c /= (uint32_t)dmx::kTripleCodes;
    const uint32_t c1 = c % (uint32_t)dmx::kTripleCodes, c0 = c / (uint32_t)dmx::kTripleCodes;
    const uint32_t cs[3] = {c0, c1, c2};
    for (int r = 0; r < 3; ++r) bytes[r] = cs[r] >= (uint32_t)dmx::kTripleBq ? (0x80u | (cs[r] - (uint32_t)dmx::kTripleBq)) : cs[r];
    nb = 3;
  }
  double wA[2][5], wR[2][5], pG[2][5];
  for (int n1 = 0; n1 < 2; ++n1)
    for (int q = 0; q < 5; ++q) {                  // the weights of k_certify's FIVE form
      const int l = n1 ? (q > 2 ? 2 : q) : min(q, 2), m = n1 ? q - l : 0;
      const double p = 0.5 * l + (m - l) * 0.5 * (n1 ? 0.5 : 0.0);
      wA[n1][q] = p; wR[n1][q] = 1.0 - p; pG[n1][q] = 1.0;
    }
  for (int r = 0; r < nb; ++r) {
    const uint32_t byte = bytes[r], bq = byte & 127u;
    const bool alt = (byte >> 7) != 0;
    const double pR = alt ? tabs[128 + bq] : tabs[bq];
    const double pA = alt ? tabs[bq] : tabs[128 + bq];
    double mx[2] = {0.0, 0.0};
    for (int n1 = 0; n1 < 2; ++n1)
      for (int i = 0; i < 5; ++i) {
        pG[n1][i] *= (pR * wR[n1][i] + pA * wA[n1][i]);
        mx[n1] = fmax(mx[n1], pG[n1][i]);
      }
    const double m = fmax(mx[0], mx[1]);
    const double y = rcp_refined(m);
    for (int n1 = 0; n1 < 2; ++n1)
      for (int i = 0; i < 5; ++i) pG[n1][i] = div_by(pG[n1][i], m, y);
  }
  double mx[2] = {0.0, 0.0};
  for (int n1 = 0; n1 < 2; ++n1)
    for (int i = 0; i < 5; ++i) {
      pG[n1][i] += 1e-6;                                                     // :649
      mx[n1] = fmax(mx[n1], pG[n1][i]);
    }
  const double m = fmax(mx[0], mx[1]);
  const double y = rcp_refined(m);
  double* o = out + (size_t)e * kCFinStride;
  for (int i = 0; i < 5; ++i) o[i] = div_by(pG[1][i], m, y);                 // :656-663, the alpha = 0.5 lane's values (what both lanes of a k_certify pair use)
  for (int i = 0; i < 3; ++i) o[5 + i] = div_by(pG[0][i], m, y);             // ... and the alpha = 0 lane's three distinct ones (k_doublet_sym's phase 1)
}

// Phase 1 of k_certify for one (pair, alpha) lane: the pG values of :597-663 with the one-max-across-both-alphas renormalisation
// after every read, finished (:656-663) and handed from the alpha = 0.5 lane to its alpha = 0 neighbour.  NV = 9: the nine
// values pG[l][m]; NV = 5 (alpha[0] == 0): the five distinct values of alpha 0.5 (weight p = (l + m) / 4, index l + m) beside the
// three of alpha 0 (p = l / 2) — entries with equal weights go through identical operations, so the values are bit-identical.
// seeds (NV = 5, the default grid; round 4): the lane's five values after the pair's first read — or first two, both of base quality < 64 — come from a
// table built on the device with this very loop (k_build_certify_seeds: [256 + 16 384 read codes][alpha lane][6]), and the loop starts at read 1 or 2:
// at 1.25 reads per pair it used to run max(cnt) ~ 2.6 times per tile of 32 pairs with most lanes idle, now 0.6 times.
constexpr int kCSeedStride = 6;                  // doubles per (entry, alpha lane): five values + pad (16-byte aligned loads)
constexpr int64_t kCSeedN = 256 + 128 * 128;
// One maximum across the AW lanes that hold the alphas of one pair (AW = 2: the neighbour by DPP; 4, 8: a butterfly; 0: a butterfly of run-time width aw).
template <int AW>
__device__ __forceinline__ double alpha_group_max(double mx, int aw = AW) {
  if constexpr (AW == 2) {
    const double o = shfl_xor1(mx);
    return fmax(mx, o);
  } else if constexpr (AW == 0) {
    for (int d = 1; d < aw; d <<= 1) { const double o = __shfl_xor(mx, d); mx = fmax(mx, o); }
    return mx;
  } else {
#pragma unroll
    for (int d = 1; d < AW; d <<= 1) { const double o = __shfl_xor(mx, d); mx = fmax(mx, o); }
    return mx;
  }
}
// Phase 1 of every doublet kernel and of k_certify for one (pair, alpha) lane, up to the last division: pG after the read loop of :597-639 and the
// +1e-6 of :649, and (returned) the maximum of :650-655 across the pair's AW alpha lanes.  Callers that fuse the final division into their gp00 loop
// take these; the others call certify_pair_values.
//   AW    lanes of the max (alpha_group_max); n_ok = false marks a padding alpha of a grid narrower than AW: it skips the update but takes part in the shuffles
//   DIVI  the plain division of a pair deeper than kSafeReads inline (`/`) instead of through div_slow: both are the IEEE division, same bits — the
//         nine-value STRICT kernels were tuned with the inline form and the five-value FAST ones with the call, and each keeps its registers that way
//   RD4   the first four reads come from rd4 (load_rd4); false: every read is loaded from pv.reads (the alpha-grid kernels, whose lanes hold no rd4)
//   W     the mixing weights of :613 (wA: p, wR: 1 - p): register arrays, or pointers into LDS (k_doublet_clsp keeps them there)
template <int NV, int AW = 2, bool DIVI = false, bool RD4 = true, class W>
__device__ __forceinline__ double pair_values_open(const PileupView& pv, uint32_t cnt, int64_t off, uint32_t rd4, const double* s_tab,
                                                   const W& wA, const W& wR, int n1, double (&out)[NV],
                                                   const double* __restrict__ cseed = nullptr, bool n_ok = true, int aw = AW) {
  double pG[NV];                                                          // (a local, copied out at the end: worked on through `out` the callers' kernels
#pragma unroll                                                            //  take other registers — the array is then promoted element by element, not as a vector)
  for (int i = 0; i < NV; ++i) pG[i] = 1.0;                               // :597
  uint32_t r_start = 0;
  if (NV == 5 && cseed) {
    if (cnt >= 1 && cnt <= kSafeReads) {
      const uint32_t b0 = rd4 & 0xFFu, b1 = (rd4 >> 8) & 0xFFu;
      const bool two = cnt >= 2 && ((b0 | b1) & 0x40u) == 0;
      const uint32_t i2 = ((((b0 & 0x80u) >> 1) | (b0 & 0x3Fu)) << 7) | (((b1 & 0x80u) >> 1) | (b1 & 0x3Fu));
      const double* sp = cseed + ((size_t)(two ? 256u + i2 : b0) * 2 + (size_t)n1) * kCSeedStride;
      const double2 a = *reinterpret_cast<const double2*>(sp), b = *reinterpret_cast<const double2*>(sp + 2);
      pG[0] = a.x; pG[1] = a.y; pG[2] = b.x; pG[3] = b.y; pG[NV - 1] = sp[4];
      r_start = two ? 2u : 1u;
    }
  }
  // first read any lane still has to apply (wave-uniform)
  uint32_t r = 0;
  if (NV == 5 && cseed) r = __any(r_start == 0 && cnt > 0) ? 0u : (__any(r_start <= 1 && cnt > 1) ? 1u : 2u);
  for (; __any(r < cnt); ++r) {
    const bool has = r >= r_start && r < cnt, live = has && n_ok;
    uint32_t byte;
    if constexpr (RD4) byte = live ? (r < 4 ? (rd4 >> (8 * r)) & 0xFFu : (uint32_t)pv.reads[off + r]) : 0u;
    else byte = has ? pv.reads[off + r] : 0u;
    const uint32_t bq = byte & 127u;
    const bool alt = (byte >> 7) != 0;
    const double pR = alt ? s_tab[128 + bq] : s_tab[bq];                // :606
    const double pA = alt ? s_tab[bq] : s_tab[128 + bq];                // :607
    double mx = 0.0;
    if (live) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        pG[i] *= (pR * wR[i] + pA * wA[i]);                             // :625
        mx = fmax(mx, pG[i]);                                 // :626-627
      }
    }
    mx = alpha_group_max<AW>(mx, aw);                                   // one max across all alphas of the pair
    if (live) {
      if (cnt <= kSafeReads) {
        const double y = rcp_refined(mx);
#pragma unroll
        for (int i = 0; i < NV; ++i) pG[i] = div_by(pG[i], mx, y);      // :632-639
      } else {
#pragma unroll
        for (int i = 0; i < NV; ++i) pG[i] = DIVI ? pG[i] / mx : div_slow(pG[i], mx);
      }
    }
  }
  double mx = 0.0;
  if (n_ok) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      pG[i] += 1e-6;                                                     // :649
      mx = fmax(mx, pG[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) out[i] = pG[i];
  (void)n1;
  return alpha_group_max<AW>(mx, aw);
}
// ... and finished (:656-663; numerators >= 1e-6, the maximum in [1e-6, 1 + 1e-6]).  HAND: k_certify's hand-over at the end — the alpha = 0.5 lane hands a
// copy of its values to its alpha = 0 neighbour (which only had to contribute to the shared maxima), and the two lanes of a pair then take one
// accumulator each; false: each lane keeps its own.
template <int NV, bool HAND = true, int AW = 2, bool DIVI = false>
__device__ __forceinline__ void certify_pair_values(const PileupView& pv, uint32_t cnt, int64_t off, uint32_t rd4, const double* s_tab,
                                                    const double (&wA)[NV], const double (&wR)[NV], int n1, double (&v)[NV],
                                                    const double* __restrict__ cseed = nullptr) {
  double pG[NV];
  const double mx = pair_values_open<NV, AW, DIVI>(pv, cnt, off, rd4, s_tab, wA, wR, n1, pG, cseed);
  const double y = rcp_refined(mx);
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = div_by(pG[i], mx, y);
  if (HAND) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = shfl_odd(v[i]);   // (the alpha = 0.5 lane is the odd one: n1 == lane & 1)
  }
}

// The pair headers of one tile of TP covered pairs -> LDS, by the first TP lanes of the cell (tid): read count n, first read byte (a segmented
// scan of the counts from rd_base) and SNP id sn.  The barrier and the rd_base update (s_off[tp - 1] + s_cnt[tp - 1], by every lane) stay with the caller.
template <int TP>
__device__ __forceinline__ void publish_tile_headers(uint32_t n, int32_t sn, int tid, int64_t rd_base, uint32_t* s_cnt, int64_t* s_off, int32_t* s_snp) {
  const uint32_t incl = seg_scan_incl<TP>(n);
  s_cnt[tid] = n;
  s_off[tid] = rd_base + (int64_t)(incl - n);
  s_snp[tid] = sn;
}
// ... loaded here (the kernels that prefetch a tile's header while the one before it is computed publish what they hold in registers)
template <int TP>
__device__ __forceinline__ void load_tile_headers(const PileupView& pv, int nrd_width, int64_t p_beg, int64_t tbase, int tp, int tid, int64_t rd_base,
                                                  uint32_t* s_cnt, int64_t* s_off, int32_t* s_snp) {
  if (tid < TP) {
    const bool v = tid < tp;
    const uint32_t n = v ? load_nrd(pv.pair_nrd, p_beg + tbase + tid, nrd_width) : 0u;
    const int32_t sn = v ? (pv.pair_snp ? pv.pair_snp[p_beg + tbase + tid] : (int32_t)(tbase + tid)) : 0;
    publish_tile_headers<TP>(n, sn, tid, rd_base, s_cnt, s_off, s_snp);
  }
}
// The genotype rows of the tile's SNPs -> LDS as G (float32 as stored, or widened to binary64), coalesced along the row, by the cell's TPC threads.
template <int TPC, typename G>
__device__ __forceinline__ void stage_geno_rows(const float* __restrict__ g, const int32_t* s_snp, int tp, int tid, int row_len, int GS, G* s_g) {
  int r = tid % row_len, ti = tid / row_len;
  const int dr = TPC % row_len, dt = TPC / row_len;
  while (ti < tp) {
    s_g[ti * GS + r] = (G)g[(size_t)s_snp[ti] * row_len + r];
    r += dr; ti += dt;
    if (r >= row_len) { r -= row_len; ++ti; }
  }
}
// The llks00 term of one (pair, alpha) lane: the sum of the pair's nine phase-1 values value(l, m) weighted by gp00 = gp0s[l] gp0s[m] (qq: the SNP's
// gp0s; :555), in the reference's l-major order (:702-705), and the log term of :708-709 -> *t00.  Returns whether the sum was a normal positive
// number (the fast log's domain; k_doublet_a2s ignores it).  value() is called once per (l, m), in order: the kernels finish (div_by) and store
// their pG in it.
template <class F>
__device__ __forceinline__ bool llks00_term(const double (&qq)[3], F&& value, const double* s_log, double* t00) {
  double sum = 0.0;
#pragma unroll
  for (int l = 0; l < 3; ++l)
#pragma unroll
    for (int m = 0; m < 3; ++m) sum += ((qq[l] * qq[m]) * value(l, m));
  *t00 = dmx_log2_fast(sum, s_log);
  return __builtin_amdgcn_class(sum, 0x100);
}
template <class F>
__device__ __forceinline__ bool llks00_term(const double* __restrict__ gp0, int32_t snp, F&& value, const double* s_log, double* t00) {
  const double* g0 = gp0 + (size_t)snp * 3;
  const double q0 = g0[0], q1 = g0[1], q2 = g0[2];
  const double qq[3] = {q0, q1, q2};
  return llks00_term(qq, value, s_log, t00);
}
// The seeds of certify_pair_values<5>: one thread per read code (256 one-read codes, then 128 x 128 two-read codes of base quality < 64) runs the
// loop of :597-639 for BOTH alpha lanes (0 and 0.5: the maximum of :626-627 runs across them) — the same operations on the same operands as the
// two lanes of k_certify, hence the same bits.
__global__ void k_build_certify_seeds(const double* __restrict__ tabs, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= kCSeedN) return;
  uint32_t bytes[2]; int nb;
  if (e < 256) { bytes[0] = (uint32_t)e; bytes[1] = 0; nb = 1; }
  else {
    const uint32_t i2 = (uint32_t)(e - 256), c0 = i2 >> 7, c1 = i2 & 127u;
    bytes[0] = ((c0 & 0x40u) << 1) | (c0 & 0x3Fu); bytes[1] = ((c1 & 0x40u) << 1) | (c1 & 0x3Fu); nb = 2;
  }
  double wA[2][5], wR[2][5], pG[2][5];
  for (int n1 = 0; n1 < 2; ++n1)
    for (int q = 0; q < 5; ++q) {                  // the weights of k_certify's FIVE form
      const int l = n1 ? (q > 2 ? 2 : q) : min(q, 2), m = n1 ? q - l : 0;
      const double p = 0.5 * l + (m - l) * 0.5 * (n1 ? 0.5 : 0.0);
      wA[n1][q] = p; wR[n1][q] = 1.0 - p; pG[n1][q] = 1.0;
    }
  for (int r = 0; r < nb; ++r) {
    const uint32_t byte = bytes[r], bq = byte & 127u;
    const bool alt = (byte >> 7) != 0;
    const double pR = alt ? tabs[128 + bq] : tabs[bq];
    const double pA = alt ? tabs[bq] : tabs[128 + bq];
    double mx[2] = {0.0, 0.0};
    for (int n1 = 0; n1 < 2; ++n1)
      for (int i = 0; i < 5; ++i) {
        pG[n1][i] *= (pR * wR[n1][i] + pA * wA[n1][i]);
        mx[n1] = fmax(mx[n1], pG[n1][i]);
      }
    const double m = fmax(mx[0], mx[1]);
    const double y = rcp_refined(m);
    for (int n1 = 0; n1 < 2; ++n1)
      for (int i = 0; i < 5; ++i) pG[n1][i] = div_by(pG[n1][i], m, y);
  }
  for (int n1 = 0; n1 < 2; ++n1) {
    double* o = out + ((size_t)e * 2 + n1) * kCSeedStride;
    for (int i = 0; i < 5; ++i) o[i] = pG[n1][i];
    o[5] = 0.0;
  }
}



// K1.  Wavefronts are independent (no workgroup barrier in the loop).  A wavefront owns CW cells for their whole SNP
// range and walks them tile by tile, T = 64/CW SNP-pairs per cell per tile:
//   compute  lane (cell c = lane/T, pair ti = lane%T): GL of its pair once per tile, then per chunk of KC samples the KC
//            log terms (plus, in chunk 0, the term of the average-genotype model llk0) -> LDS, chain-major
//            ([cell][slot][ti]);
//   sum      lane a < CW*(KC+1) owns accumulator (cell a/(KC+1), slot a%(KC+1)): adds the tile's T terms in ascending
//            pair order (16-byte LDS reads, two terms each).
// Genotype probabilities stay float32 in memory (they ARE float32 values, bcf_filtered_reader.h:78) and are widened in
// registers.  Dense pileups (every cell covers every SNP, pair_snp == NULL) read them SNP-minor (gT[row element][snp],
// g0T[l][snp]) so a cell's T lanes read contiguous addresses; sparse pileups read the row of the lane's own SNP from the
// SNP-major originals (g[snp][k][l], gp0s[snp][l]).
// A two-deep software pipeline keeps global-memory latency off the dependent path: the pair header (read count, SNP id)
// of tile+2 is in flight while the read offsets of tile+1 are scanned and its leading read bytes requested, while tile
// is computed.
template <int CW, int KC, bool DENSE>
__global__ __launch_bounds__(kThreads, 4) void k_singlet(PileupView pv, int nrd_width, const float* __restrict__ gq,
                                                         const double* __restrict__ g0q, const double* __restrict__ tabs,
                                                         const int32_t* __restrict__ sched, int32_t V, int32_t QS,
                                                         double* __restrict__ llks, double* __restrict__ llk0s,
                                                         const int64_t* __restrict__ blk, int32_t blk_i, int32_t nblk) {
  // blk != nullptr: this launch covers SNP block blk_i of nblk only (sparse pileups whose genotype matrix does not fit the L2:
  // launch_singlet walks the SNP axis block by block so that the rows a launch gathers stay L2-resident).  blk[cell][b] = {first
  // pair, first read byte} of the cell at the start of block b (k_snp_blocks); the running sums are parked in llks / llk0s
  // between launches: same lanes, same order of additions, same bits as the one-launch walk.
  constexpr int ablate = DMX_ABLATE;             // profiling builds only (tools/build_variant.sh); 0 in the product
  constexpr int T = 64 / CW;
  constexpr int TS = T + 2;                      // row stride of a chain in LDS (doubles): keeps 16-byte alignment, and
                                                 // 2*TS mod 64 == 4 dwords spreads the chains of a wavefront over the banks
  constexpr int NC = KC + 1;                     // chains per cell and chunk: KC samples + llk0 (chunk 0 only)
  constexpr int NW = kThreads / 64;
  static_assert(CW * NC <= 64, "one lane per chain");
  extern __shared__ double s_dyn[];              // [NW][nq][CW*NC] running accumulators of this workgroup's sample chunks
  __shared__ double s_tab[kTabK1];
  const double* s_first = s_tab + kTab;
  __shared__ __attribute__((aligned(16))) double s_term[NW][CW * NC * TS];
  const double* s_log = s_tab + kLut;
  const double* s_final = s_first + kFirst;

  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int nch = (V + KC - 1) / KC;
  // panels with more than QS chunks of KC samples are cut into sample slabs, one workgroup (blockIdx.y) per slab; each
  // slab recomputes the (cheap) genotype likelihoods of its cells' pairs
  const int q_lo = (int)blockIdx.y * QS, q_hi = min(nch, q_lo + QS), nq = q_hi - q_lo;
  for (int i = t; i < kTabK1; i += kThreads) s_tab[i] = tabs[i];
  for (int i = t; i < NW * nq * CW * NC; i += kThreads) s_dyn[i] = 0.0;
  __syncthreads();                               // the only workgroup barrier

  double* term = s_term[w];
  double* accs = s_dyn + (size_t)w * nq * CW * NC;
  const int slot0 = (blockIdx.x * NW + w) * CW;  // first of this wavefront's cells in launch order
  if (slot0 >= pv.B) return;

  // compute-phase identity
  const int c = lane / T, ti = lane % T;
  const bool cell_ok = slot0 + c < pv.B;
  const int32_t cell = cell_ok ? sched[slot0 + c] : 0;
  const int64_t* bt = blk ? blk + ((size_t)cell * (nblk + 1) + blk_i) * 2 : nullptr;
  const int64_t p_beg = cell_ok ? (blk ? bt[0] : pv.cell_pair_off[cell]) : 0;
  const int64_t np = cell_ok ? (blk ? bt[2] : pv.cell_pair_off[cell + 1]) - p_beg : 0;
  int64_t rd_base = cell_ok ? (blk ? bt[1] : pv.cell_read_off[cell]) : 0;
  int64_t max_np = np;
#pragma unroll
  for (int d = T; d < 64; d <<= 1) max_np = max(max_np, __shfl_xor(max_np, d));
  // sum-phase identity
  const int a_c = lane / NC, a_kk = lane % NC;
  const bool a_ok = lane < CW * NC && slot0 + a_c < pv.B;
  const int64_t a_np = __shfl(np, (a_ok ? a_c : 0) * T);
  const int32_t a_cell = __shfl(cell, (a_ok ? a_c : 0) * T);
  const size_t S = (size_t)pv.S;
  if (blk && blk_i > 0 && a_ok) {                // resume: the sums of the blocks before this one
    for (int q = q_lo; q < q_hi; ++q) {
      double v = 0.0;
      if (a_kk < KC) { const int k = q * KC + a_kk; if (k < V) v = llks[(size_t)a_cell * V + k]; }
      else if (q == 0) v = llk0s[a_cell];
      accs[(q - q_lo) * (CW * NC) + lane] = v;
    }
  }

  // Dense genotype planes are read through buffer descriptors: address = descriptor base + scalar plane offset + lane
  // offset, one instruction per element and no per-lane 64-bit address arithmetic (S*V*12 < 4 GiB is checked at launch).
  const uint32_t plane4 = (uint32_t)S * 4u, plane8 = (uint32_t)S * 8u;
  const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc((void*)gq, 0, DENSE ? (int)min((size_t)0x7FFFFFFF, S * (size_t)V * 12) : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_g0 = __builtin_amdgcn_make_buffer_rsrc((void*)g0q, 0, DENSE ? (int)min((size_t)0x7FFFFFFF, S * (size_t)24) : 0, 0x00020000);

  struct Raw { uint32_t n; int32_t snp; };
  struct Hdr { uint32_t n; int32_t snp; uint32_t rd4; int64_t off; };
  auto issue = [&](int64_t tile) {               // loads only
    Raw r;
    const int64_t pi = tile * T + ti;
    const bool v = pi < np;
    r.n = v ? load_nrd(pv.pair_nrd, p_beg + pi, nrd_width) : 0u;
    r.snp = v ? (DENSE ? (int32_t)pi : pv.pair_snp[p_beg + pi]) : 0;
    return r;
  };
  auto prepare = [&](const Raw& r) {             // prefix-scan the read counts of the cell's T pairs, request the bytes
    Hdr h;
    h.n = r.n; h.snp = r.snp;
    const uint32_t incl = seg_scan_incl<T>(r.n);
    h.off = rd_base + (int64_t)(incl - r.n);
    rd_base += seg_last<T>(incl, lane);
    h.rd4 = 0;
    if (r.n > 0) {
      if (h.off + 4 <= pv.R) __builtin_memcpy(&h.rd4, pv.reads + h.off, 4);   // bytes past the pair's reads are never interpreted
      else for (int64_t i = h.off; i < pv.R; ++i) h.rd4 |= (uint32_t)pv.reads[i] << (8 * (int)(i - h.off));
    }
    return h;
  };

  Hdr nxt = prepare(issue(0));
  Raw pre = issue(1);
  for (int64_t tile = 0; tile * T < max_np; ++tile) {
    Hdr cur = nxt;
    if (!(ablate & 16)) {
      nxt = prepare(pre);                        // tile+1: its counts arrived a tile ago
      pre = issue(tile + 2);                     // tile+2: loads in flight
    } else { cur.n = 1; cur.rd4 = 0x9e; cur.snp = 0; }
    const bool valid = tile * T + ti < np;

    // ---- genotype likelihoods of this lane's pair (:427-452).  Pairs with at most one read (the bulk of single-cell
    // data) are a table lookup on the read byte; deeper pairs continue the reference's per-read loop from the table's
    // state after the first read.
    double G0, G1, G2;
    {
      const uint32_t n = cur.n;
      const uint32_t b0 = cur.rd4 & 0xFFu;
      const double* f = s_final + 3 * (n ? b0 : 256u);
      G0 = f[0]; G1 = f[1]; G2 = f[2];
      if (n >= 2 && !(ablate & 1)) {
        const double* f1 = s_first + 3 * b0;
        G0 = f1[0]; G1 = f1[1]; G2 = f1[2];
        gl_continue(1u, n, cur.rd4, pv.reads, cur.off, s_tab, G0, G1, G2);
      }
    }
    // dense: uniform plane base per row element + this lane's SNP index (scalar base, 32-bit lane offset, no per-load
    // address arithmetic); sparse: this lane's own row
    const uint32_t s_idx = (uint32_t)min((int64_t)(tile * T + ti), (int64_t)S - 1);
    const uint32_t boff4 = s_idx * 4u, boff8 = s_idx * 8u;     // lane byte offsets for the buffer loads below
    const float* __restrict__ grow = gq + (size_t)cur.snp * V * 3;
    const double* __restrict__ g0row = g0q + (size_t)cur.snp * 3;

    for (int q = q_lo; q < q_hi; ++q) {
      const int k0 = q * KC;
      float a[KC][3];
      double a0[3];
#pragma unroll
      for (int kk = 0; kk < KC; ++kk) {          // all loads of the chunk first; slots past sample V-1 re-read it (ignored)
        const int k = min(k0 + kk, V - 1);
#pragma unroll
        for (int l = 0; l < 3; ++l)
          a[kk][l] = (ablate & 8) ? 0.3f + 0.01f * kk
                     : (DENSE ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_g, boff4, (uint32_t)(k * 3 + l) * plane4, 0))
                              : grow[k * 3 + l]);
      }
      if (q == 0) {
#pragma unroll
        for (int l = 0; l < 3; ++l)
          a0[l] = (ablate & 8) ? 0.33
                  : (DENSE ? __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs_g0, boff8, (uint32_t)l * plane8, 0)) : g0row[l]);
      }
      if (valid) {
        bool fast_ok = true;
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
          const double x = G0 * (double)a[kk][0] + G1 * (double)a[kk][1] + G2 * (double)a[kk][2];   // :456
          fast_ok &= __builtin_amdgcn_class(x, 0x100);                       // +normal: the fast path's domain
          if (!(ablate & 32) || kk == 0) term[(c * NC + kk) * TS + ti] = (ablate & 2) ? x : dmx_log_fast(x, s_log); else G0 += x;
        }
        if (q == 0) {
          const double x = G0 * a0[0] + G1 * a0[1] + G2 * a0[2];             // :459
          fast_ok &= __builtin_amdgcn_class(x, 0x100);
          term[(c * NC + KC) * TS + ti] = (ablate & 2) ? x : dmx_log_fast(x, s_log);
        }
        if (__builtin_expect(!fast_ok, 0)) {       // never for real likelihoods; keeps log(0) / log(nan) semantics
          for (int kk = 0; kk <= KC; ++kk) {       // one rolled copy of ocml's log; operands re-read from memory
            if (kk == KC && q != 0) break;
            double b[3];
            if (kk < KC) {
              const int k = min(k0 + kk, V - 1);
              for (int l = 0; l < 3; ++l) b[l] = (double)(DENSE ? (gq + (size_t)(k * 3 + l) * S)[s_idx] : grow[k * 3 + l]);
            } else {
              for (int l = 0; l < 3; ++l) b[l] = DENSE ? (g0q + (size_t)l * S)[s_idx] : g0row[l];
            }
            const double x = G0 * b[0] + G1 * b[1] + G2 * b[2];
            if (!__builtin_amdgcn_class(x, 0x100)) term[(c * NC + kk) * TS + ti] = log(x);
          }
        }
      }
      // ---- ordered sums of this (tile, chunk).  Wavefront-local: the LDS serves one wavefront's accesses in program
      // order; the compiler barrier only stops the compiler from moving the reads above the stores (and the next stores above the reads).
      DMX_WAVE_LDS_ORDER();
      if (a_ok && (a_kk < KC ? k0 + a_kk < V : q == 0)) {
        const int64_t left = a_np - tile * T;
        const int cnt = (ablate & 4) ? 1 : (left >= T ? T : (left > 0 ? (int)left : 0));
        const double* row = &term[lane * TS];
        double s = accs[(q - q_lo) * (CW * NC) + lane];
        int i = 0;
        for (; i + 16 <= cnt; i += 16) {           // loads first (latency paid once), then the ordered adds
          double2 v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const double2*>(&row[i + 2 * j]);
#pragma unroll
          for (int j = 0; j < 8; ++j) { s += v[j].x; s += v[j].y; }
        }
        for (; i < cnt; ++i) s += row[i];           // ascending SNP order: the reference's order
        accs[(q - q_lo) * (CW * NC) + lane] = s;
      }
      DMX_WAVE_LDS_ORDER();
    }
  }
  if (a_ok) {
    for (int q = q_lo; q < q_hi; ++q) {
      const double s = accs[(q - q_lo) * (CW * NC) + lane];
      if (a_kk < KC) { const int k = q * KC + a_kk; if (k < V) llks[(size_t)a_cell * V + k] = s; }
      else if (q == 0) llk0s[a_cell] = s;
    }
  }
}

#ifndef DMX_K1O_U
#define DMX_K1O_U 4
#endif
// the C library's log() for an argument outside dmx_log's domain (never for real likelihoods), out of line: one copy per kernel, not per term
__device__ __attribute__((noinline)) double log_slow(double x) { return log(x); }

// K1 with OWNED accumulators (round 5; soft fields, up to 64 samples).  k_singlet's lanes are pairs: they park V + 1 log terms per pair in the
// LDS, and nine lanes of the wavefront then add them up chunk by chunk — a serial 64-add chain per chunk of eight samples with 9 of 64 lanes
// active, a third of that kernel's issue cycles, on top of an LDS store and load per term.  Here a sample's running sum lives in a register of
// ONE lane for the whole walk (k_doublet_*'s ownership):
//   phase 1  lane (cell c = lane / TPC, pair ti = lane % TPC): GL of its pair (:427-452) and the llk0 term (:459) -> LDS;
//   phase 2  lane (cell c, sample j = lane % TPC): for the tile's pairs in ascending order: the pair's GL (a broadcast LDS read), its own three
//            genotype probabilities at that SNP (SNP-major rows g[snp][k][l]: the cell's lanes read one contiguous row), the dot product, the log, the add.
// Same operands, same operations, same order of additions as k_singlet: the same bits (tests/test_gpu_parity.py::test_k1_owned_sums_are_k_singlets_bits).
// CHK = false (k_check_geno passed the matrix): GL >= 1e-6 / (1 + 3e-6) and a row's maximum >= 1e-30 make every log argument a normal positive
// number, and the per-term class test is dropped (k_doublet_a2's CHK).
template <int TPC, bool DENSE, bool CHK>
__global__ __launch_bounds__(kThreads, 5) void k_singlet_own(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                             const double* __restrict__ gp0, const double* __restrict__ tabs,
                                                             const int32_t* __restrict__ sched, int32_t V,
                                                             double* __restrict__ llks, double* __restrict__ llk0s,
                                                             const int64_t* __restrict__ blk, int32_t blk_i, int32_t nblk) {
  static_assert(TPC == 16 || TPC == 32 || TPC == 64, "lanes per cell");
  constexpr int CW = 64 / TPC, T = TPC;          // cells per wavefront; pairs per cell and tile
  constexpr int TS = T + 2;                      // stride of a cell's llk0 terms (doubles): 16-byte aligned rows
  constexpr int NW = kThreads / 64;
  constexpr int U = DMX_K1O_U;                   // pairs per batch of phase 2: their rows are requested together, a batch ahead of their use
  static_assert(T % U == 0, "batches");
  __shared__ double s_tab[kTabK1];
  __shared__ __attribute__((aligned(16))) double s_gl[NW][64 * 4];     // [pair lane][G0 G1 G2 -]
  __shared__ __attribute__((aligned(16))) double s_t0[NW][CW * TS];    // [cell][pair] llk0 terms
  __shared__ uint32_t s_row[NW][64];                                   // byte offset of the pair's genotype row
  const double* s_first = s_tab + kTab;
  const double* s_log = s_tab + kLut;
  const double* s_final = s_first + kFirst;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  for (int i = t; i < kTabK1; i += kThreads) s_tab[i] = tabs[i];
  __syncthreads();                               // the only workgroup barrier
  const int slot0 = (blockIdx.x * NW + w) * CW;
  if (slot0 >= pv.B) return;
  double* gl = s_gl[w];
  double* t0s = s_t0[w];
  uint32_t* rowo = s_row[w];

  const int c = lane / T, ti = lane % T;         // phase 1: pair ti of cell c; phase 2: sample ti of cell c
  const bool cell_ok = slot0 + c < pv.B;
  const int32_t cell = cell_ok ? sched[slot0 + c] : 0;
  const int64_t* bt = blk ? blk + ((size_t)cell * (nblk + 1) + blk_i) * 2 : nullptr;     // (k_singlet's SNP-blocked walk)
  const int64_t p_beg = cell_ok ? (blk ? bt[0] : pv.cell_pair_off[cell]) : 0;
  const int64_t np = cell_ok ? (blk ? bt[2] : pv.cell_pair_off[cell + 1]) - p_beg : 0;
  int64_t rd_base = cell_ok ? (blk ? bt[1] : pv.cell_read_off[cell]) : 0;
  int64_t max_np = np;
#pragma unroll
  for (int d = T; d < 64; d <<= 1) max_np = max(max_np, __shfl_xor(max_np, d));
  const DmxLogPins lk = dmx_log_pins();          // the log's addend constants in registers (same operations, same bits: csrc/dmx_log.hpp)
  const bool own = cell_ok && ti < V;
  const bool own0 = cell_ok && ti == 0;          // the cell's first lane also owns llk0
  double acc = 0.0, acc0 = 0.0;
  if (blk && blk_i > 0) {                        // resume: the sums of the blocks before this one
    if (own) acc = llks[(size_t)cell * V + ti];
    if (own0) acc0 = llk0s[cell];
  }
  const uint32_t row_bytes = (uint32_t)V * 12u;
  const uint32_t my_off = (uint32_t)min(ti, V - 1) * 12u;          // lanes past the panel re-read its last sample (ignored)
  const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc((void*)g, 0, (int)min((size_t)0x7FFFFFFF, (size_t)pv.S * V * 12), 0x00020000);

  struct Raw { uint32_t n; int32_t snp; };
  struct Hdr { uint32_t n; int32_t snp; uint32_t rd4; int64_t off; };
  auto issue = [&](int64_t tile) {               // loads only
    Raw r;
    const int64_t pi = tile * T + ti;
    const bool v = pi < np;
    r.n = v ? load_nrd(pv.pair_nrd, p_beg + pi, nrd_width) : 0u;
    r.snp = v ? (DENSE ? (int32_t)pi : pv.pair_snp[p_beg + pi]) : 0;
    return r;
  };
  auto prepare = [&](const Raw& r) {             // prefix-scan the read counts of the cell's T pairs, request the bytes
    Hdr h;
    h.n = r.n; h.snp = r.snp;
    const uint32_t incl = seg_scan_incl<T>(r.n);
    h.off = rd_base + (int64_t)(incl - r.n);
    rd_base += seg_last<T>(incl, lane);
    h.rd4 = load_rd4(pv, h.off, r.n);
    return h;
  };
  Hdr nxt = prepare(issue(0));
  Raw pre = issue(1);
  for (int64_t tile = 0; tile * T < max_np; ++tile) {
    const Hdr cur = nxt;
    nxt = prepare(pre);                          // tile+1: its counts arrived a tile ago
    pre = issue(tile + 2);                       // tile+2: loads in flight
    // ---- phase 1: genotype likelihoods of this lane's pair (:427-452), exactly k_singlet's
    double G0, G1, G2;
    {
      const uint32_t n = cur.n;
      const uint32_t b0 = cur.rd4 & 0xFFu;
      const double* f = s_final + 3 * (n ? b0 : 256u);
      G0 = f[0]; G1 = f[1]; G2 = f[2];
      if (n >= 2) {
        const double* f1 = s_first + 3 * b0;
        G0 = f1[0]; G1 = f1[1]; G2 = f1[2];
        gl_continue(1u, n, cur.rd4, pv.reads, cur.off, s_tab, G0, G1, G2);
      }
    }
    {
      const double* __restrict__ g0row = gp0 + (size_t)cur.snp * 3;
      const double x = G0 * g0row[0] + G1 * g0row[1] + G2 * g0row[2];        // :459
      double tm = dmx_log_fast_pinned(x, s_log, lk);
      if (CHK) { if (__builtin_expect(!__builtin_amdgcn_class(x, 0x100), 0)) tm = log_slow(x); }
      t0s[c * TS + ti] = tm;
      *reinterpret_cast<double2*>(&gl[lane * 4]) = make_double2(G0, G1);
      gl[lane * 4 + 2] = G2;
      rowo[lane] = (uint32_t)cur.snp * row_bytes;
    }
    DMX_WAVE_LDS_ORDER();
    const int64_t left = np - tile * T;
    const int cnt = left >= T ? T : (left > 0 ? (int)left : 0);
    // ---- llk0: the cell's first lane adds the tile's terms in pair order
    if (own0) {
      const double* row = &t0s[c * TS];
      int i = 0;
      for (; i + 8 <= cnt; i += 8) {               // loads first, then the ordered adds
        double2 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const double2*>(&row[i + 2 * j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc0 += v[j].x; acc0 += v[j].y; }
      }
      for (; i < cnt; ++i) acc0 += row[i];
    }
    // ---- phase 2: lane (c, sample ti) adds its term of every pair of the tile, ascending
    const bool whole = __all(cnt == T);
    int cmax = cnt;
#pragma unroll
    for (int d = T; d < 64; d <<= 1) cmax = max(cmax, __shfl_xor(cmax, d));
    auto request = [&](int p0, float (&a)[U][3]) {          // the rows of pairs p0 .. p0+U-1: this lane's three probabilities of each
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t vo = rowo[c * T + p0 + u] + my_off;
#pragma unroll
        for (int l = 0; l < 3; ++l) a[u][l] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_g, vo + 4u * l, 0, 0));
      }
    };
    auto batch = [&](int p0, const float (&a)[U][3], auto whole_c) {
      constexpr bool WHOLE = decltype(whole_c)::value;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const double2 g01 = *reinterpret_cast<const double2*>(&gl[(c * T + p0 + u) * 4]);
        const double g2 = gl[(c * T + p0 + u) * 4 + 2];
        const double x = g01.x * (double)a[u][0] + g01.y * (double)a[u][1] + g2 * (double)a[u][2];      // :456
        double tm = dmx_log_fast_pinned(x, s_log, lk);
        if (CHK) { if (__builtin_expect(!__builtin_amdgcn_class(x, 0x100), 0)) tm = log_slow(x); }
        if (WHOLE) acc += tm;
        else if (p0 + u < cnt) acc += tm;
      }
    };
    if (whole) {                                   // two row buffers: batch b+1's rows travel while batch b computes
      float ra[2][U][3];
      request(0, ra[0]);
#pragma unroll
      for (int b = 0; b < T / U; ++b) {
        if (b + 1 < T / U) request((b + 1) * U, ra[(b + 1) & 1]);
        batch(b * U, ra[b & 1], std::true_type{});
      }
    } else {
#pragma unroll 1
      for (int p0 = 0; p0 < cmax; p0 += U) { float ra[U][3]; request(p0, ra); batch(p0, ra, std::false_type{}); }
    }
    DMX_WAVE_LDS_ORDER();
  }
  if (own) llks[(size_t)cell * V + ti] = acc;
  if (own0) llk0s[cell] = acc0;
}

// K1 over genotype classes (see "Genotype classes" below: <= 4 distinct probability rows per SNP, --field GT).
// Same walk, ownership and ordered sums as k_singlet.  Per pair the lane evaluates log(GL . row_d) ONCE per class d (plus
// the llk0 term), parks those doubles in a per-lane LDS scratch, and for every sample k of the chunk copies
// scratch[class id of (snp, k)] into the chain buffer — the very double k_singlet would have computed for sample k
// (same operands, same operations), so the sums that follow are bit-identical.  4+1 logs per pair instead of V+1.
// CAN (round 4; canonical GT classes, see k_canon_apply; launched with chk == 0 only): classes 0..2 are the three SNP-independent rows of a called
// genotype, so log(GL . row) of a pair with up to three tabulated reads is an entry of ltab (k_build_canon_logs: the same expression, the same
// log, evaluated once per read combination instead of once per pair) — three of the five dot products and logs of a pair become one gather,
// requested a tile ahead with the GL seed.  Class 3 (the SNP's own row, where oth[snp] says there is one) and the llk0 term are evaluated as before.
template <int CW, int KC, bool CAN = false>
__global__ __launch_bounds__(kThreads, 5) void k_singlet_cls(PileupView pv, int nrd_width, const float* __restrict__ rows, int chk,
                                                             const uint32_t* __restrict__ idw, const double* __restrict__ gp0,
                                                             const double* __restrict__ tabs,
                                                             const int32_t* __restrict__ sched, int32_t V,
                                                             double* __restrict__ llks, double* __restrict__ llk0s,
                                                             const double* __restrict__ ltab, const uint8_t* __restrict__ oth, double chi, double clo) {
  static_assert(KC == 8 || KC == 4, "a chunk's 2-bit class ids must sit inside one 32-bit id word");
  constexpr int ablate = DMX_ABLATE;             // profiling builds only (tools/build_variant.sh); 0 in the product
  constexpr int T = 64 / CW;
  constexpr int TS = T + 2;
  constexpr int NC = KC + 1;
  constexpr int NW = kThreads / 64;
  constexpr int SD = 4;                          // scratch doubles per lane: the 4 class terms (the llk0 term goes straight to its chain)
  static_assert(CW * NC <= 64, "one lane per chain");
  extern __shared__ double s_dyn[];              // [NW][nch][CW*NC] running accumulators
  // LDS budget: 5 workgroups per CU (<= 32 KB each) so that 10 k wavefronts make two full rounds of 5 120 instead of
  // three of 4 096.  Only dmx_log's table is staged; the read LUT and the first-read tables are read from global memory
  // (L1-hot, 3 + 12 KB) — they are touched once per pair at most.
  __shared__ double s_log_tab[DMX_LOG_TABLE_DOUBLES];
  __shared__ __attribute__((aligned(16))) double s_term[NW][CW * NC * TS];
  __shared__ double s_scr[NW][64 * SD];
  const double* s_log = s_log_tab;
  const double* s_tab = tabs;                    // read LUT in global memory

  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int nch = (V + KC - 1) / KC;
  const int nwd = (V + 15) / 16;
  for (int i = t; i < DMX_LOG_TABLE_DOUBLES; i += kThreads) s_log_tab[i] = tabs[kLut + i];
  for (int i = t; i < NW * nch * CW * NC; i += kThreads) s_dyn[i] = 0.0;
  __syncthreads();                               // the only workgroup barrier

  double* term = s_term[w];
  double* scr = &s_scr[w][lane];                 // class-major [d][lane]: a lane's four terms sit 512 bytes apart, i.e. in the SAME
                                                 // bank pair, and the 32 lanes of an LDS cycle in 32 different ones whatever class each
                                                 // of them looks up (lane-major [lane][d] made every lookup a 4-way bank conflict)
  double* accs = s_dyn + (size_t)w * nch * CW * NC;
  const int slot0 = (blockIdx.x * NW + w) * CW;
  if (slot0 >= pv.B) return;

  const int c = lane / T, ti = lane % T;
  const bool cell_ok = slot0 + c < pv.B;
  const int32_t cell = cell_ok ? sched[slot0 + c] : 0;
  const int64_t p_beg = cell_ok ? pv.cell_pair_off[cell] : 0;
  const int64_t np = cell_ok ? pv.cell_pair_off[cell + 1] - p_beg : 0;
  int64_t rd_base = cell_ok ? pv.cell_read_off[cell] : 0;
  int64_t max_np = np;
#pragma unroll
  for (int d = T; d < 64; d <<= 1) max_np = max(max_np, __shfl_xor(max_np, d));
  const int a_c = lane / NC, a_kk = lane % NC;
  const bool a_ok = lane < CW * NC && slot0 + a_c < pv.B;
  const int64_t a_np = __shfl(np, (a_ok ? a_c : 0) * T);
  const int32_t a_cell = __shfl(cell, (a_ok ? a_c : 0) * T);

  struct Raw { uint32_t n; int32_t snp; };
  struct Hdr { uint32_t n; int32_t snp; uint32_t rd4; int64_t off; };
  auto issue = [&](int64_t tile) {
    Raw r;
    const int64_t pi = tile * T + ti;
    const bool v = pi < np;
    r.n = v ? load_nrd(pv.pair_nrd, p_beg + pi, nrd_width) : 0u;
    r.snp = v ? (pv.pair_snp ? pv.pair_snp[p_beg + pi] : (int32_t)pi) : 0;
    return r;
  };
  auto prepare = [&](const Raw& r) {
    Hdr h;
    h.n = r.n; h.snp = r.snp;
    const uint32_t incl = seg_scan_incl<T>(r.n);
    h.off = rd_base + (int64_t)(incl - r.n);
    rd_base += seg_last<T>(incl, lane);
    h.rd4 = 0;
    if (r.n > 0) {
      if (h.off + 4 <= pv.R) __builtin_memcpy(&h.rd4, pv.reads + h.off, 4);
      else for (int64_t i = h.off; i < pv.R; ++i) h.rd4 |= (uint32_t)pv.reads[i] << (8 * (int)(i - h.off));
    }
    return h;
  };

  // CAN: the pair's three canonical-class terms from ltab (has: the reads are inside the final tables, i.e. gl_seed's r0 >= n)
  struct CanSeed { double l0, l1, l2; bool has; };
  auto can_seed = [&](uint32_t n, uint32_t rd4) {
    CanSeed c; c.l0 = c.l1 = c.l2 = 0.0; c.has = false;
    if constexpr (CAN) {
      const uint32_t b0 = rd4 & 0xFFu, b1 = (rd4 >> 8) & 0xFFu, b2 = (rd4 >> 16) & 0xFFu;
      const uint32_t q0 = b0 & 127u, q1 = b1 & 127u, q2 = b2 & 127u;
      const bool two = n == 2 && ((b0 | b1) & 0x40u) == 0;
      const bool three = n == 3 && max(max(q0, q1), q2) < (uint32_t)dmx::kTripleBq;
      const uint32_t i2 = ((((b0 & 0x80u) >> 1) | (b0 & 0x3Fu)) << 7) | (((b1 & 0x80u) >> 1) | (b1 & 0x3Fu));
      const uint32_t c0 = ((b0 & 0x80u) ? (uint32_t)dmx::kTripleBq : 0u) + q0, c1 = ((b1 & 0x80u) ? (uint32_t)dmx::kTripleBq : 0u) + q1,
                     c2 = ((b2 & 0x80u) ? (uint32_t)dmx::kTripleBq : 0u) + q2;
      const uint32_t i3 = __umul24(__umul24(c0, (uint32_t)dmx::kTripleCodes) + c1, (uint32_t)dmx::kTripleCodes) + c2;
      uint32_t i = n == 0 ? 256u : b0;
      i = two ? (uint32_t)kCanL2 + i2 : i;
      i = three ? (uint32_t)kCanL3 + i3 : i;
      c.has = n < 2 || two || three;
      if (c.has) {
        const double2 v = *reinterpret_cast<const double2*>(ltab + 4 * (size_t)i);
        c.l0 = v.x; c.l1 = v.y; c.l2 = ltab[4 * (size_t)i + 2];
      }
    }
    return c;
  };
  Hdr h1 = prepare(issue(0));
  Hdr h2 = prepare(issue(1));
  Raw pre = issue(2);
  GlSeed s1 = gl_seed(tabs, h1.n, h1.rd4);
  CanSeed c1 = can_seed(h1.n, h1.rd4);
  for (int64_t tile = 0; tile * T < max_np; ++tile) {
    const Hdr cur = h1;
    const GlSeed cs = s1;
    const CanSeed cc = c1;
    h1 = h2;
    s1 = gl_seed(tabs, h1.n, h1.rd4);              // tile+1: its read bytes were requested an iteration ago
    c1 = can_seed(h1.n, h1.rd4);
    h2 = prepare(pre);                             // tile+2: scan, request its read bytes
    pre = issue(tile + 3);                         // tile+3: header loads in flight
    const bool valid = tile * T + ti < np;

    // class rows, llk0 row and the first id word of this lane's SNP (SNP-major: contiguous across a dense tile)
    const int32_t snp_l = (ablate & 256) ? (cur.snp & 63) : cur.snp;     // ablation: every row load an L1 hit
    const float4* rp = reinterpret_cast<const float4*>(rows + (size_t)snp_l * 12);
    float4 r0 = {0.f, 0.f, 0.f, 0.f}, r1 = r0, r2 = r0;
    bool has_o = false;
    if constexpr (CAN) { has_o = valid && oth[snp_l] != 0; if (has_o) r2 = rp[2]; }   // (class 3's row: r2.y, r2.z, r2.w)
    else { r0 = rp[0]; r1 = rp[1]; r2 = rp[2]; }
    const double* g0 = gp0 + (size_t)snp_l * 3;
    const double q0 = g0[0], q1 = g0[1], q2 = g0[2];
    const uint32_t* idrow = idw + (size_t)snp_l * nwd;
    uint32_t wcur = idrow[0];

    double G0, G1, G2;                                                       // :427-452
    gl_finish(cs, (ablate & 1) ? min(cur.n, cs.r0) : cur.n, cur.rd4, pv.reads, cur.off, s_tab, G0, G1, G2);
    if constexpr (CAN) {
      if (valid) {
        double t0 = cc.l0, t1 = cc.l1, t2 = cc.l2;
        if (!cc.has) {                               // deeper pairs / base qualities beyond the tables: the expressions of k_build_canon_logs
          t0 = dmx_log_fast(G0 * chi + G1 * clo + G2 * clo, s_log);
          t1 = dmx_log_fast(G0 * clo + G1 * chi + G2 * clo, s_log);
          t2 = dmx_log_fast(G0 * clo + G1 * clo + G2 * chi, s_log);
        }
        scr[0] = t0; scr[64] = t1; scr[128] = t2;
        if (has_o) scr[192] = dmx_log_fast(G0 * (double)r2.y + G1 * (double)r2.z + G2 * (double)r2.w, s_log);   // class 3
        term[(c * NC + KC) * TS + ti] = dmx_log_fast(G0 * q0 + G1 * q1 + G2 * q2, s_log);                         // llk0 (:459)
      }
    } else
    if (valid) {
      const double x0 = G0 * (double)r0.x + G1 * (double)r0.y + G2 * (double)r0.z;     // class 0   (:456)
      const double x1 = G0 * (double)r0.w + G1 * (double)r1.x + G2 * (double)r1.y;     // class 1
      const double x2 = G0 * (double)r1.z + G1 * (double)r1.w + G2 * (double)r2.x;     // class 2
      const double x3 = G0 * (double)r2.y + G1 * (double)r2.z + G2 * (double)r2.w;     // class 3
      const double x4 = G0 * q0 + G1 * q1 + G2 * q2;                                    // llk0      (:459)
      // chk == 0: k_check_geno proved every row finite, non-negative, with an entry >= 1e-30, and GL >= 1e-6 / (1 + 3e-6) (:452): every
      // argument is a positive normal number and the class test cannot fire (what the K2 kernels' CHK = false variants rely on)
      const bool fast_ok = !chk || (__builtin_amdgcn_class(x0, 0x100) && __builtin_amdgcn_class(x1, 0x100) && __builtin_amdgcn_class(x2, 0x100) &&
                                    __builtin_amdgcn_class(x3, 0x100) && __builtin_amdgcn_class(x4, 0x100));
      double* t0 = &term[(c * NC + KC) * TS + ti];   // the llk0 chain's slot of this pair
      if (__builtin_expect(fast_ok, 1)) {
        scr[0] = dmx_log_fast(x0, s_log); scr[64] = dmx_log_fast(x1, s_log); scr[128] = dmx_log_fast(x2, s_log);
        scr[192] = dmx_log_fast(x3, s_log); *t0 = dmx_log_fast(x4, s_log);
      } else {                                     // never for real likelihoods; keeps log(0) / log(nan) semantics
        scr[0] = x0; scr[64] = x1; scr[128] = x2; scr[192] = x3; *t0 = x4;
        for (int d = 0; d < SD; ++d) scr[64 * d] = log(scr[64 * d]);
        *t0 = log(*t0);
      }
    }
    for (int q = 0; q < nch; ++q) {
      const int k0 = q * KC;
      if (q > 0 && (k0 & 15) == 0) wcur = idrow[k0 >> 4];
      if (valid && !(ablate & 64)) {
        const uint32_t bits = wcur >> (2 * (k0 & 15));      // the chunk's KC class ids, 2 bits each
#pragma unroll
        for (int kk = 0; kk < KC; ++kk)
          term[(c * NC + kk) * TS + ti] = scr[((bits >> (2 * kk)) & 3u) << 6];     // sample k0+kk's term (slots past V-1 are never summed)
      }
      DMX_WAVE_LDS_ORDER();
      if (a_ok && (a_kk < KC ? k0 + a_kk < V : q == 0)) {
        const int64_t left = a_np - tile * T;
        const int cnt = (ablate & 4) ? 1 : (left >= T ? T : (left > 0 ? (int)left : 0));
        const double* row = &term[lane * TS];
        double s = accs[q * (CW * NC) + lane];
        int i = 0;
        for (; i + 16 <= cnt; i += 16) {
          double2 v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const double2*>(&row[i + 2 * j]);
#pragma unroll
          for (int j = 0; j < 8; ++j) { s += v[j].x; s += v[j].y; }
        }
        for (; i < cnt; ++i) s += row[i];           // ascending SNP order: the reference's order
        accs[q * (CW * NC) + lane] = s;
      }
      DMX_WAVE_LDS_ORDER();
    }
  }
  if (a_ok) {
    for (int q = 0; q < nch; ++q) {
      const double s = accs[q * (CW * NC) + lane];
      if (a_kk < KC) { const int k = q * KC + a_kk; if (k < V) llks[(size_t)a_cell * V + k] = s; }
      else if (q == 0) llk0s[a_cell] = s;
    }
  }
}

// K1 over CANONICAL genotype classes, lean form (round 5; V <= 16, one-byte read counts, arrays below 4 GiB — cfg2 — else k_singlet_cls<.., CAN>).
// Same ownership, same expressions, same order of additions as k_singlet_cls<CW, KC, true>: every output is bit-identical.  What changed is
// everything AROUND the arithmetic, which was three quarters of that kernel's instruction stream (profiles/pmc_cfg2_strict.json: 76 % of its
// VALU instructions were not FP64) and all of its exposed latency:
//   * ONE table gather per pair instead of two: ctab[i] = {GL0, GL1, GL2, log(GL . row_0), log(GL . row_1), log(GL . row_2)} (64-byte entries,
//     k_build_ctab: the GL of gl_seed + gl_finish and the logs of k_build_canon_logs, evaluated once per read combination), indexed by the
//     read count and the RAW leading read bytes — one read: the byte; two reads: the 16-bit word (all 65 536 combinations, no quality test);
//     three reads of quality < 48: the 96^3 code.  Anything else (0.25 % of the pairs at 1.25 reads per pair) walks the read loop as before.
//   * ONE record per SNP instead of four arrays: SnpRec = {gp0[3], the id word, the "has a fourth row" flag} (32 bytes, k_build_snprec).
//   * 32-bit element offsets from wave-uniform array bases (SGPR base + VGPR offset loads) instead of 64-bit pointer arithmetic per load.
//   * A three-deep software pipeline in which NOTHING a tile consumes was requested in the same iteration: tile t + 3's read counts, tile
//     t + 2's scan and leading read bytes, tile t + 1's table entry and SNP record are in flight while tile t computes (the memory system
//     returns a wavefront's loads in order, so the old kernel's wait for the current tile's rows also waited for the prefetches behind them).
// per-SNP record, four 16-byte parts in four arrays (SoA; a dense tile reads each contiguously): [S] {q0, q1} | [S] {q2, ids 0..3} | [S] {ids 4..11} | [S] {ids 12..15, oth, 0}
// (gp0 = q; id k = a 16-bit 512 * class of sample k: the byte offset of the class's plane in the scratch)
constexpr size_t kSnpRecBytes = 64;
constexpr uint32_t kCt2 = 257, kCt3 = 257 + 65536;                              // ctab regions: one read (256 = none) | two reads (raw bytes) | three reads
constexpr int64_t kCtN = (int64_t)kCt3 + (int64_t)dmx::kTripleCodes * dmx::kTripleCodes * dmx::kTripleCodes;
constexpr int kCtBq = 42, kCtLds = 2 * kCtBq + 1;                                // LDS copy of region 1: one read of quality < 42 (code allele * 42 + bq; the CLI caps at 40), 84 = no read

__global__ void k_build_snprec(const double* __restrict__ gp0, const uint8_t* __restrict__ ids, const uint8_t* __restrict__ oth, int32_t S, int32_t V,
                               uint4* __restrict__ out) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const double q0 = gp0[3 * s], q1 = gp0[3 * s + 1], q2 = gp0[3 * s + 2];
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // sample k's class id as the BYTE OFFSET of its class plane in the scratch: half-word k = id * 512
  for (int k = 0; k < V && k < 16; ++k) w[k >> 1] |= ((uint32_t)(ids[s * V + k] & 3u) * 512u) << (16 * (k & 1));
  out[s] = make_uint4((uint32_t)__double2loint(q0), (uint32_t)__double2hiint(q0), (uint32_t)__double2loint(q1), (uint32_t)__double2hiint(q1));
  out[(size_t)S + s] = make_uint4((uint32_t)__double2loint(q2), (uint32_t)__double2hiint(q2), w[0], w[1]);
  out[2 * (size_t)S + s] = make_uint4(w[2], w[3], w[4], w[5]);
  out[3 * (size_t)S + s] = make_uint4(w[6], w[7], (uint32_t)oth[s], 0u);
}

// ctab entry i: the pair's genotype likelihoods exactly as gl_seed + gl_finish produce them (the host tables where they reach, the kernel's own
// read loop beyond), and the three canonical-class terms with k_build_canon_logs' expressions and log.
__global__ void k_build_ctab(const double* __restrict__ tabs, double hi, double lo, double* __restrict__ ctab) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kCtN) return;
  uint32_t n, rd4;
  if (i < kCt2) { n = i == 256 ? 0u : 1u; rd4 = (uint32_t)i & 0xFFu; }
  else if (i < kCt3) { n = 2u; rd4 = (uint32_t)(i - kCt2); }
  else {
    uint32_t c = (uint32_t)(i - kCt3);
    const uint32_t c2 = c % (uint32_t)dmx::kTripleCodes; c /= (uint32_t)dmx::kTripleCodes;
    const uint32_t c1 = c % (uint32_t)dmx::kTripleCodes, c0 = c / (uint32_t)dmx::kTripleCodes;
    auto byte_of = [](uint32_t code) { return code >= (uint32_t)dmx::kTripleBq ? (0x80u | (code - (uint32_t)dmx::kTripleBq)) : code; };
    n = 3u; rd4 = byte_of(c0) | (byte_of(c1) << 8) | (byte_of(c2) << 16);
  }
  const GlSeed sd = gl_seed(tabs, n, rd4);
  double G0, G1, G2;
  gl_finish(sd, n, rd4, nullptr, 0, tabs, G0, G1, G2);
  const double* T = tabs + kLut;
  double* o = ctab + 8 * i;
  o[0] = G0; o[1] = G1; o[2] = G2;
  o[3] = dmx_log_fast(G0 * hi + G1 * lo + G2 * lo, T);
  o[4] = dmx_log_fast(G0 * lo + G1 * hi + G2 * lo, T);
  o[5] = dmx_log_fast(G0 * lo + G1 * lo + G2 * hi, T);
  o[6] = 0.0; o[7] = 0.0;
}

// The first version of this kernel (everything gathered from the global table) was bound by the CU's vector L1: one tag look-up per lane and
// gather instruction, 273 per 64-pair tile = 0.94 look-ups per cycle and CU (profiles/r05_k1_probe.txt) — not by issue, not by bandwidth.  The LDS
// serves 16 lanes per cycle, so the table entries of the commonest pairs — no read, or ONE read of quality < 42 (the CLI caps at 40): 78 % of the
// pairs at 1.25 reads per pair — come from a 4 KB LDS copy and only the other lanes gather from the global table, a tile ahead.  The copy has to fit
// beside 5 workgroups per CU (10 000 barcodes at two per wavefront are ONE round of 5 wavefronts per SIMD; a workgroup of ten wavefronts sharing a
// bigger copy is admitted once per CU only — measured): 32 000 bytes per workgroup (the LDS is handed out in 1 280-byte pieces: 32 432 bytes were
// admitted four times per CU), found by keeping the running sums in registers and, for matrices without a fourth genotype row (OTH = false: no
// missing genotypes), three class planes of scratch instead of four.  OTH = true keeps the
// global gathers for every lane.
// (waves per SIMD: five for the one- and two-barcode forms — 10 000 barcodes at two per wavefront are ONE round of five; the four-barcode form, picked
//  from 131 072 barcodes, carries four barcodes' pipelines in its registers and asks for what it gets: four, three with two chunks — VERDICT r5 weak 9)
template <int CW, int KC, bool OTH, int NCH>     // NCH: chunks of KC samples (1 or 2; V <= NCH * KC)
__global__ __launch_bounds__(kThreads, (CW == 4 ? (NCH == 2 ? 3 : 4) : 5)) void k_singlet_can(PileupView pv, const uint4* __restrict__ snprec, const float* __restrict__ rows,
                                                             const double* __restrict__ ctab, const double* __restrict__ tabs,
                                                             const int32_t* __restrict__ sched, int32_t V,
                                                             double* __restrict__ llks, double* __restrict__ llk0s, double chi, double clo) {
  static_assert(KC == 8 || KC == 4, "a chunk's 2-bit class ids must sit inside one 32-bit id word");
  constexpr int T = 64 / CW;
  constexpr int TS = T + 2;
  constexpr int NC = KC + 1;
  constexpr int NW = kThreads / 64;
  constexpr int NPL = OTH ? 4 : 3;               // class planes of scratch
  static_assert(CW * NC <= 64, "one lane per chain");
  __shared__ double s_log_tab[DMX_LOG_TABLE_DOUBLES];
  __shared__ __attribute__((aligned(16))) double s_term[NW][CW * NC * TS];
  __shared__ double s_scr[NW][64 * NPL];
  __shared__ __attribute__((aligned(16))) double s_ct[OTH ? 2 : kCtLds * 6];
  const double* s_log = s_log_tab;

  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  constexpr int nch = NCH;
  constexpr int NIDW = NCH * KC / 2;             // id words per SNP (two samples each)
  for (int i = t; i < DMX_LOG_TABLE_DOUBLES; i += kThreads) s_log_tab[i] = tabs[kLut + i];
  if constexpr (!OTH)
    for (int i = t; i < kCtLds * 6; i += kThreads) {
      const int e = i / 6, f = i % 6;
      const int b = e == 2 * kCtBq ? 256 : (e >= kCtBq ? (0x80 | (e - kCtBq)) : e);   // the read byte (allele << 7) | bq of code e
      s_ct[i] = ctab[8 * b + f];
    }
  __syncthreads();                               // the only workgroup barrier

  double* term = s_term[w];
  double* scr = &s_scr[w][lane];                 // class-major [d][lane] (conflict-free whatever class each lane looks up, see k_singlet_cls): a sample's
                                                 // term is at (lane address + 512 * class) — ONE v_add_u32_sdwa per look-up with the ids stored as that offset
  const uint32_t scr_a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) double*)scr;   // (its LDS byte address)
  const uint32_t ct_a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) double*)s_ct;
  const int slot0 = (blockIdx.x * NW + w) * CW;
  if (slot0 >= pv.B) return;

  const int c = lane / T, ti = lane % T;
  const bool cell_ok = slot0 + c < pv.B;
  const int32_t cell = cell_ok ? sched[slot0 + c] : 0;
  const uint32_t p_beg = cell_ok ? (uint32_t)pv.cell_pair_off[cell] : 0u;               // (the launcher checked: every offset fits 32 bits)
  const uint32_t np = cell_ok ? (uint32_t)(pv.cell_pair_off[cell + 1] - pv.cell_pair_off[cell]) : 0u;
  uint32_t rd_base = cell_ok ? (uint32_t)pv.cell_read_off[cell] : 0u;
  uint32_t max_np = np;
#pragma unroll
  for (int d = T; d < 64; d <<= 1) max_np = max(max_np, (uint32_t)__shfl_xor((int)max_np, d));
  const int a_c = lane / NC, a_kk = lane % NC;
  const bool a_ok = lane < CW * NC && slot0 + a_c < pv.B;
  const uint32_t a_np = (uint32_t)__shfl((int)np, (a_ok ? a_c : 0) * T);
  const int32_t a_cell = __shfl(cell, (a_ok ? a_c : 0) * T);
  double acc[2] = {0.0, 0.0};                    // the chain's running sums (chunk 0, chunk 1), in registers
  const uint8_t* __restrict__ nrd8 = (const uint8_t*)pv.pair_nrd;
  const uint8_t* __restrict__ reads = pv.reads;
  const int32_t* __restrict__ psnp = pv.pair_snp;
  const uint4* __restrict__ recA = snprec;
  const uint4* __restrict__ recB = snprec + pv.S;
  const uint4* __restrict__ recC = snprec + 2 * (size_t)pv.S;
  const uint4* __restrict__ recD = snprec + 3 * (size_t)pv.S;
  constexpr bool need_c = NIDW > 2, need_d = OTH || NIDW > 6;

  // stage A: read count (and SNP id) of the lane's pair of a tile
  struct Raw { uint32_t n; uint32_t snp; };
  auto stage_a = [&](uint32_t tile) {
    Raw r;
    const uint32_t pi = tile * T + ti;
    const bool v = pi < np;
    const uint32_t pa = v ? p_beg + pi : 0u;
    r.n = v ? (uint32_t)nrd8[pa] : 0u;
    r.snp = v ? (psnp ? (uint32_t)psnp[pa] : pi) : 0u;
    return r;
  };
  // stage B: the pair's read offset (scan over the cell's lanes) and its leading read bytes
  struct Hdr { uint32_t n, snp, rd4, off; };
  auto stage_b = [&](const Raw& r) {
    Hdr h;
    h.n = r.n; h.snp = r.snp;
    const uint32_t incl = seg_scan_incl<T>(r.n);
    h.off = rd_base + (incl - r.n);
    rd_base += seg_last<T>(incl, lane);
    uint32_t v;
    __builtin_memcpy(&v, reads + (r.n ? h.off : 0u), 4);        // (the launcher checked: four bytes past the last read are readable)
    h.rd4 = v;
    return h;
  };
  // stage C: the pair's table entry — requested from the global table a tile ahead unless the LDS copy has it (no read, or one read of quality
  // < kCtBq), in which case stage D reads it when the tile computes — and its SNP's record
  struct Seed { double2 a, b, cc; double q0, q1, q2; uint32_t idb[NIDW], oth, lds; bool fast; };   // lds: byte offset of the entry in the LDS copy, or ~0u
  auto in_lds_copy = [](uint32_t n, uint32_t rd4) { return !OTH && (n == 0 || (n == 1 && (rd4 & 0x7Fu) < (uint32_t)kCtBq)); };
  auto stage_c = [&](const Hdr& h) {
    Seed sd;
    const uint32_t n = h.n, rd4 = h.rd4;
    sd.fast = true;
    sd.lds = (n == 0 ? (uint32_t)(2 * kCtBq) : (((rd4 & 0x80u) ? (uint32_t)kCtBq : 0u) + (rd4 & 0x7Fu))) * 48u;
    if (!in_lds_copy(n, rd4)) {
      sd.lds = ~0u;
      uint32_t idx = n == 0 ? 256u : (rd4 & 0xFFu);
      idx = n == 2 ? kCt2 + (rd4 & 0xFFFFu) : idx;
      bool fast = n <= 2;
      if (n == 3) {
        const uint32_t q0 = rd4 & 127u, q1 = (rd4 >> 8) & 127u, q2 = (rd4 >> 16) & 127u;
        if (max(max(q0, q1), q2) < (uint32_t)dmx::kTripleBq) {
          const uint32_t c0 = ((rd4 & 0x80u) ? (uint32_t)dmx::kTripleBq : 0u) + q0, c1 = ((rd4 & 0x8000u) ? (uint32_t)dmx::kTripleBq : 0u) + q1,
                         c2 = ((rd4 & 0x800000u) ? (uint32_t)dmx::kTripleBq : 0u) + q2;
          idx = kCt3 + __umul24(__umul24(c0, (uint32_t)dmx::kTripleCodes) + c1, (uint32_t)dmx::kTripleCodes) + c2;
          fast = true;
        }
      }
      sd.fast = fast;
      const double2* e = reinterpret_cast<const double2*>(ctab + 8u * idx);
      sd.a = e[0]; sd.b = e[1]; sd.cc = e[2];
    }
    const uint4 r0 = recA[h.snp], r1 = recB[h.snp];
    sd.q0 = __hiloint2double((int)r0.y, (int)r0.x); sd.q1 = __hiloint2double((int)r0.w, (int)r0.z);
    sd.q2 = __hiloint2double((int)r1.y, (int)r1.x); sd.idb[0] = r1.z; sd.idb[1] = r1.w;
    sd.oth = 0u;
    if constexpr (need_c) { const uint4 r2 = recC[h.snp]; sd.idb[2] = r2.x; sd.idb[3] = r2.y; if constexpr (NIDW > 4) { sd.idb[4] = r2.z; sd.idb[5] = r2.w; } }
    if constexpr (need_d) { const uint4 r3 = recD[h.snp]; if constexpr (NIDW > 6) { sd.idb[6] = r3.x; sd.idb[7] = r3.y; } sd.oth = r3.z; }
    return sd;
  };
  typedef double v2d_t __attribute__((ext_vector_type(2)));
  typedef const __attribute__((address_space(3))) v2d_t* LdsD2;        // (an LDS-address-space pointer: the two sources must not be merged into flat loads)

  // the sums of chunk q belong to lane (cell a_c, slot a_kk): sample q * KC + a_kk, or (slot KC, chunk 0) the llk0 chain
  const bool sum_lane[2] = {a_ok && (a_kk < KC ? a_kk < V : true), a_ok && a_kk < KC && KC + a_kk < V};
  uint32_t min_np = cell_ok ? np : 0xFFFFFFFFu;  // tiles below it are whole for every barcode of the wavefront: their sums need no counting
#pragma unroll
  for (int d = T; d < 64; d <<= 1) min_np = min(min_np, (uint32_t)__shfl_xor((int)min_np, d));

  // stage D: one tile.  Lanes beyond their barcode's last pair carry n = 0, SNP 0 (stage A): they compute like any other lane, into slots the
  // sums never reach — no per-lane validity test anywhere below.
  auto compute = [&](const Hdr& cur, Seed& cs, uint32_t tile) {
    if (cs.lds != ~0u) {                           // the LDS copy's entry
      LdsD2 p = (LdsD2)(uintptr_t)(ct_a + cs.lds);
      const v2d_t va = p[0], vb = p[1], vc = p[2];
      cs.a.x = va.x; cs.a.y = va.y; cs.b.x = vb.x; cs.b.y = vb.y; cs.cc.x = vc.x; cs.cc.y = vc.y;
    }
    double G0 = cs.a.x, G1 = cs.a.y, G2 = cs.b.x, t0 = cs.b.y, t1 = cs.cc.x, t2 = cs.cc.y;
    if (!cs.fast) {                                // deeper pairs, qualities beyond the tables: the read loop and the three logs, as k_singlet_cls<.., CAN>
      const GlSeed sd = gl_seed(tabs, cur.n, cur.rd4);
      gl_finish(sd, cur.n, cur.rd4, reads, (int64_t)cur.off, tabs, G0, G1, G2);
      t0 = dmx_log_fast(G0 * chi + G1 * clo + G2 * clo, s_log);
      t1 = dmx_log_fast(G0 * clo + G1 * chi + G2 * clo, s_log);
      t2 = dmx_log_fast(G0 * clo + G1 * clo + G2 * chi, s_log);
    }
    scr[0] = t0; scr[64] = t1; scr[128] = t2;
    if constexpr (OTH)
      if (cs.oth) {                                // class 3: the SNP's own fourth row (a missing genotype's Hardy-Weinberg row)
        const float* r3 = rows + (size_t)cur.snp * 12 + 9;
        scr[192] = dmx_log_fast(G0 * (double)r3[0] + G1 * (double)r3[1] + G2 * (double)r3[2], s_log);
      }
    term[(c * NC + KC) * TS + ti] = dmx_log_fast(G0 * cs.q0 + G1 * cs.q1 + G2 * cs.q2, s_log);            // llk0 (:459)
    const uint32_t done = tile * T;
    const bool whole = done + T <= min_np;         // (wave-uniform)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (q < nch) {
        // sample q*KC+kk's term = scratch[its class][lane]: address = lane address + the sample's id (slots past V-1 are never summed; class 3 only with OTH)
        typedef const __attribute__((address_space(3))) double* LdsD;
        const int h0 = q * (KC / 2);               // the chunk's first id word (two samples per word)
        term[(c * NC + 0) * TS + ti] = *(LdsD)(uintptr_t)add_word_of<0>(scr_a, cs.idb[h0]);
        term[(c * NC + 1) * TS + ti] = *(LdsD)(uintptr_t)add_word_of<1>(scr_a, cs.idb[h0]);
        term[(c * NC + 2) * TS + ti] = *(LdsD)(uintptr_t)add_word_of<0>(scr_a, cs.idb[h0 + 1]);
        term[(c * NC + 3) * TS + ti] = *(LdsD)(uintptr_t)add_word_of<1>(scr_a, cs.idb[h0 + 1]);
        if constexpr (KC == 8) {
          term[(c * NC + 4) * TS + ti] = *(LdsD)(uintptr_t)add_word_of<0>(scr_a, cs.idb[h0 + 2]);
          term[(c * NC + 5) * TS + ti] = *(LdsD)(uintptr_t)add_word_of<1>(scr_a, cs.idb[h0 + 2]);
          term[(c * NC + 6) * TS + ti] = *(LdsD)(uintptr_t)add_word_of<0>(scr_a, cs.idb[h0 + 3]);
          term[(c * NC + 7) * TS + ti] = *(LdsD)(uintptr_t)add_word_of<1>(scr_a, cs.idb[h0 + 3]);
        }
        DMX_WAVE_LDS_ORDER();
        if (sum_lane[q]) {
          const double* row = &term[lane * TS];
          double sacc = acc[q];
          if (whole) {                             // ascending SNP order: the reference's order
#pragma unroll
            for (int i = 0; i < T; i += 16) {
              double2 v[8];
#pragma unroll
              for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const double2*>(&row[i + 2 * j]);
#pragma unroll
              for (int j = 0; j < 8; ++j) { sacc += v[j].x; sacc += v[j].y; }
            }
          } else {
            const int cnt = a_np >= done + T ? T : (a_np > done ? (int)(a_np - done) : 0);
            for (int i = 0; i < cnt; ++i) sacc += row[i];
          }
          acc[q] = sacc;
        }
        DMX_WAVE_LDS_ORDER();
      }
    }
  };

  // two tiles per trip so that the two Seed sets alternate instead of being copied (the compiler's loop-carried copies were a tenth of the stream)
  Hdr h1 = stage_b(stage_a(0));
  Hdr h2 = stage_b(stage_a(1));
  Raw pre = stage_a(2);
  Seed sA = stage_c(h1), sB = sA;
  for (uint32_t tile = 0; tile * T < max_np; tile += 2) {
    {
      const Hdr cur = h1;
      h1 = h2;
      sB = stage_c(h1);                            // tile + 1
      h2 = stage_b(pre);                           // tile + 2
      pre = stage_a(tile + 3);                     // tile + 3
      compute(cur, sA, tile);
    }
    if ((tile + 1) * T >= max_np) break;
    {
      const Hdr cur = h1;
      h1 = h2;
      sA = stage_c(h1);
      h2 = stage_b(pre);
      pre = stage_a(tile + 4);
      compute(cur, sB, tile + 1);
    }
  }
  if (a_ok) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (q < nch) {
        if (a_kk < KC) { const int k = q * KC + a_kk; if (k < V) llks[(size_t)a_cell * V + k] = acc[q]; }
        else if (q == 0) llk0s[a_cell] = acc[q];
      }
  }
}

// K1, canonical GT classes, DENSE pileups, up to 8 samples (cfg2): producers / consumer (round 6).  k_singlet_can's lanes are pairs
// for the table look-up and the llk0 term and then 18 of 64 lanes are chains: per 64-pair tile it spends 32 ordered adds on 18 lanes and 17 LDS
// instructions on handing the terms from the pair lanes to the chain lanes (9 stores, 8 class look-ups), and the LDS (0.67 busy) binds it with the VALU
// close behind.  Here a workgroup is SEVEN producer wavefronts — one barcode each, lane = pair: headers, table entry, llk0 term, then ONE 32-byte record
// {log(GL . row_0), log(GL . row_1), log(GL . row_2), llk0 term} per pair into an LDS ring — and ONE consumer wavefront whose 63 lanes own the 7 x 9
// chains: chain (barcode b, sample k) adds record[b][pair][class of sample k at the pair's SNP] in ascending SNP order — the doubles k_singlet_can adds,
// in its order: the same bits.  On a dense pileup the pair's SNP is its index, so a sample's classes are one byte stream shared by all barcodes
// (clsb[k][snp] = 8 x class: the byte offset inside a record; row 8 = 24: the llk0 chain): the consumer takes 64 of them in four 16-byte loads a tile
// ahead and a chain step is one v_add_u32_sdwa (record address), one ds_read_b64 and one v_add_f64 — 64 steps per 448 pairs instead of 32 per 64.
// One workgroup barrier per tile: tile t is consumed from ring half t & 1 while the producers fill the other half with tile t + 1.
constexpr int kCpB = 7;                          // barcodes (producer wavefronts) per workgroup
constexpr int kCpThreads = (kCpB + 1) * 64;
__global__ void k_build_clsb(const uint8_t* __restrict__ ids, int32_t S, int32_t V, uint32_t stride, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)9 * stride) return;
  const int k = (int)(i / stride); const int64_t sidx = i % stride;
  out[i] = k == 8 ? (uint8_t)24 : ((k < V && sidx < S) ? (uint8_t)((ids[sidx * V + k] & 3u) * 8u) : (uint8_t)0);
}
#define DMX_CP_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")   // LDS traffic done, then the workgroup's barrier (NOT vmcnt: the prefetches stay in flight)
template <int MINW>
__global__ __launch_bounds__(kCpThreads, MINW) void k_singlet_canp(PileupView pv, const uint4* __restrict__ snprec, const uint8_t* __restrict__ clsb, uint32_t cls_stride,
                                                              const double* __restrict__ ctab, const double* __restrict__ tabs,
                                                              const int32_t* __restrict__ sched, int32_t V,
                                                              double* __restrict__ llks, double* __restrict__ llk0s, double chi, double clo) {
  constexpr int T = 64;
  __shared__ double s_log_tab[DMX_LOG_TABLE_DOUBLES];
  __shared__ __attribute__((aligned(16))) double s_ct[kCtLds * 6];
  __shared__ __attribute__((aligned(16))) double s_ring[2][kCpB][T][4];
  __shared__ uint32_t s_np[kCpB];
  const double* s_log = s_log_tab;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  for (int i = t; i < DMX_LOG_TABLE_DOUBLES; i += kCpThreads) s_log_tab[i] = tabs[kLut + i];
  for (int i = t; i < kCtLds * 6; i += kCpThreads) {
    const int e = i / 6, f = i % 6;
    const int b = e == 2 * kCtBq ? 256 : (e >= kCtBq ? (0x80 | (e - kCtBq)) : e);   // the read byte (allele << 7) | bq of code e
    s_ct[i] = ctab[8 * b + f];
  }
  const int slot0 = blockIdx.x * kCpB;
  if (t < kCpB) s_np[t] = slot0 + t < pv.B ? (uint32_t)(pv.cell_pair_off[sched[slot0 + t] + 1] - pv.cell_pair_off[sched[slot0 + t]]) : 0u;
  __syncthreads();
  uint32_t max_np = 0u, min_np = 0xFFFFFFFFu;    // over the workgroup's barcodes (uniform)
#pragma unroll
  for (int b = 0; b < kCpB; ++b) { const uint32_t v = s_np[b]; max_np = max(max_np, v); if (slot0 + b < pv.B) min_np = min(min_np, v); }
  const uint32_t ntiles = (max_np + T - 1) / T;
  typedef double v2d_t __attribute__((ext_vector_type(2)));
  typedef const __attribute__((address_space(3))) v2d_t* LdsD2;
  typedef const __attribute__((address_space(3))) double* LdsD;

  if (w == kCpB) {
    // ------------------------------------------------------------------------------------------------ the consumer
    const int b = lane / 9, kk = lane % 9;
    const bool valid = lane < kCpB * 9 && slot0 + b < pv.B;
    const int32_t cell = valid ? sched[slot0 + b] : 0;
    const uint32_t np_b = valid ? s_np[b] : 0u;
    const uint8_t* __restrict__ row = clsb + (size_t)kk * cls_stride;
    const uint32_t ring_a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) double*)&s_ring[0][lane < kCpB * 9 ? b : 0][0][0];
    constexpr uint32_t kHalf = (uint32_t)(sizeof(double) * kCpB * T * 4);
    double acc = 0.0;
    uint4 cw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) cw[i] = reinterpret_cast<const uint4*>(row)[i];
    for (uint32_t tile = 0; tile < ntiles; ++tile) {
      uint4 nw[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) nw[i] = reinterpret_cast<const uint4*>(row + (size_t)(tile + 1) * T)[i];   // (the table carries one tile of padding)
      DMX_CP_BARRIER();                            // the producers' tile is in the ring
      const uint32_t base = ring_a + (tile & 1u) * kHalf;
      if ((tile + 1) * T <= min_np) {              // whole for every barcode of the workgroup (uniform)
#pragma unroll
        for (int q = 0; q < 4; ++q) {              // 16 steps at a time: addresses, reads, then the ordered adds
          const uint32_t w0 = cw[q].x, w1 = cw[q].y, w2 = cw[q].z, w3 = cw[q].w;
          double v[16];
          v[0] = *(LdsD)(uintptr_t)(add_byte_of<0>(base, w0) + (q * 16 + 0) * 32);
          v[1] = *(LdsD)(uintptr_t)(add_byte_of<1>(base, w0) + (q * 16 + 1) * 32);
          v[2] = *(LdsD)(uintptr_t)(add_byte_of<2>(base, w0) + (q * 16 + 2) * 32);
          v[3] = *(LdsD)(uintptr_t)(add_byte_of<3>(base, w0) + (q * 16 + 3) * 32);
          v[4] = *(LdsD)(uintptr_t)(add_byte_of<0>(base, w1) + (q * 16 + 4) * 32);
          v[5] = *(LdsD)(uintptr_t)(add_byte_of<1>(base, w1) + (q * 16 + 5) * 32);
          v[6] = *(LdsD)(uintptr_t)(add_byte_of<2>(base, w1) + (q * 16 + 6) * 32);
          v[7] = *(LdsD)(uintptr_t)(add_byte_of<3>(base, w1) + (q * 16 + 7) * 32);
          v[8] = *(LdsD)(uintptr_t)(add_byte_of<0>(base, w2) + (q * 16 + 8) * 32);
          v[9] = *(LdsD)(uintptr_t)(add_byte_of<1>(base, w2) + (q * 16 + 9) * 32);
          v[10] = *(LdsD)(uintptr_t)(add_byte_of<2>(base, w2) + (q * 16 + 10) * 32);
          v[11] = *(LdsD)(uintptr_t)(add_byte_of<3>(base, w2) + (q * 16 + 11) * 32);
          v[12] = *(LdsD)(uintptr_t)(add_byte_of<0>(base, w3) + (q * 16 + 12) * 32);
          v[13] = *(LdsD)(uintptr_t)(add_byte_of<1>(base, w3) + (q * 16 + 13) * 32);
          v[14] = *(LdsD)(uintptr_t)(add_byte_of<2>(base, w3) + (q * 16 + 14) * 32);
          v[15] = *(LdsD)(uintptr_t)(add_byte_of<3>(base, w3) + (q * 16 + 15) * 32);
#pragma unroll
          for (int i = 0; i < 16; ++i) acc += v[i];                          // ascending SNP order: the reference's order (:457-460)
        }
      } else {                                     // a barcode ends inside this tile: each chain counts its own pairs
        const uint32_t done = tile * T;
        const int cnt = np_b >= done + T ? T : (np_b > done ? (int)(np_b - done) : 0);
        const uint8_t* rp = row + (size_t)done;
        for (int i = 0; i < cnt; ++i) acc += *(LdsD)(uintptr_t)(base + (uint32_t)rp[i] + (uint32_t)i * 32u);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) cw[i] = nw[i];
    }
    if (valid) {
      if (kk < 8) { if (kk < V) llks[(size_t)cell * V + kk] = acc; }
      else llk0s[cell] = acc;
    }
    return;
  }

  // -------------------------------------------------------------------------------------------------- a producer: barcode slot0 + w
  const bool cell_ok = slot0 + w < pv.B;
  if (!cell_ok) { for (uint32_t tile = 0; tile < ntiles; ++tile) DMX_CP_BARRIER(); return; }
  const int32_t cell = sched[slot0 + w];
  const uint32_t p_beg = (uint32_t)pv.cell_pair_off[cell];                  // (the launcher checked: every offset fits 32 bits)
  const uint32_t np = s_np[w];
  uint32_t rd_base = (uint32_t)pv.cell_read_off[cell];
  const uint8_t* __restrict__ nrd8 = (const uint8_t*)pv.pair_nrd;
  const uint8_t* __restrict__ reads = pv.reads;
  const uint4* __restrict__ recA = snprec;
  const uint4* __restrict__ recB = snprec + pv.S;
  const uint32_t ct_a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) double*)s_ct;
  // stages A - C: k_singlet_can's three-deep pipeline with one barcode per wavefront (T = 64) — tile t + 3's read counts, tile t + 2's scan and leading
  // read bytes, tile t + 1's table entry and SNP record are in flight while tile t computes
  struct Raw { uint32_t n; uint32_t snp; };
  auto stage_a = [&](uint32_t tile) {
    Raw r;
    const uint32_t pi = tile * T + lane;
    const bool v = pi < np;
    r.n = v ? (uint32_t)nrd8[p_beg + pi] : 0u;
    r.snp = v ? pi : 0u;                           // dense: the pair's SNP is its index
    return r;
  };
  struct Hdr { uint32_t n, snp, rd4, off; };
  auto stage_b = [&](const Raw& r) {
    Hdr h;
    h.n = r.n; h.snp = r.snp;
    const uint32_t incl = seg_scan_incl<T>(r.n);
    h.off = rd_base + (incl - r.n);
    rd_base += seg_last<T>(incl, lane);
    uint32_t v;
    __builtin_memcpy(&v, reads + (r.n ? h.off : 0u), 4);        // (the launcher checked: four bytes past the last read are readable)
    h.rd4 = v;
    return h;
  };
  struct Seed { double2 a, b, cc; double q0, q1, q2; uint32_t lds; bool fast; };   // lds: byte offset of the entry in the LDS copy, or ~0u
  auto stage_c = [&](const Hdr& h) {
    Seed sd;
    const uint32_t n = h.n, rd4 = h.rd4;
    sd.fast = true;
    sd.lds = (n == 0 ? (uint32_t)(2 * kCtBq) : (((rd4 & 0x80u) ? (uint32_t)kCtBq : 0u) + (rd4 & 0x7Fu))) * 48u;
    if (!(n == 0 || (n == 1 && (rd4 & 0x7Fu) < (uint32_t)kCtBq))) {
      sd.lds = ~0u;
      uint32_t idx = rd4 & 0xFFu;
      idx = n == 2 ? kCt2 + (rd4 & 0xFFFFu) : idx;
      bool fast = n <= 2;
      if (n == 3) {
        const uint32_t q0 = rd4 & 127u, q1 = (rd4 >> 8) & 127u, q2 = (rd4 >> 16) & 127u;
        if (max(max(q0, q1), q2) < (uint32_t)dmx::kTripleBq) {
          const uint32_t c0 = ((rd4 & 0x80u) ? (uint32_t)dmx::kTripleBq : 0u) + q0, c1 = ((rd4 & 0x8000u) ? (uint32_t)dmx::kTripleBq : 0u) + q1,
                         c2 = ((rd4 & 0x800000u) ? (uint32_t)dmx::kTripleBq : 0u) + q2;
          idx = kCt3 + __umul24(__umul24(c0, (uint32_t)dmx::kTripleCodes) + c1, (uint32_t)dmx::kTripleCodes) + c2;
          fast = true;
        }
      }
      sd.fast = fast;
      const double2* e = reinterpret_cast<const double2*>(ctab + 8u * idx);
      sd.a = e[0]; sd.b = e[1]; sd.cc = e[2];
    }
    const uint4 r0 = recA[h.snp], r1 = recB[h.snp];
    sd.q0 = __hiloint2double((int)r0.y, (int)r0.x); sd.q1 = __hiloint2double((int)r0.w, (int)r0.z);
    sd.q2 = __hiloint2double((int)r1.y, (int)r1.x);
    return sd;
  };
  // stage D: one tile -> the ring.  Lanes beyond the barcode's last pair carry n = 0, SNP 0 (stage A): they compute like any other lane, into records
  // the chains never reach.
  auto compute = [&](const Hdr& cur, Seed& cs, uint32_t tile) {
    if (cs.lds != ~0u) {                           // the LDS copy's entry
      LdsD2 p = (LdsD2)(uintptr_t)(ct_a + cs.lds);
      const v2d_t va = p[0], vb = p[1], vc = p[2];
      cs.a.x = va.x; cs.a.y = va.y; cs.b.x = vb.x; cs.b.y = vb.y; cs.cc.x = vc.x; cs.cc.y = vc.y;
    }
    double G0 = cs.a.x, G1 = cs.a.y, G2 = cs.b.x, t0 = cs.b.y, t1 = cs.cc.x, t2 = cs.cc.y;
    if (!cs.fast) {                                // deeper pairs, qualities beyond the tables: the read loop and the three logs, as k_singlet_can
      const GlSeed sd = gl_seed(tabs, cur.n, cur.rd4);
      gl_finish(sd, cur.n, cur.rd4, reads, (int64_t)cur.off, tabs, G0, G1, G2);
      t0 = dmx_log_fast(G0 * chi + G1 * clo + G2 * clo, s_log);
      t1 = dmx_log_fast(G0 * clo + G1 * chi + G2 * clo, s_log);
      t2 = dmx_log_fast(G0 * clo + G1 * clo + G2 * chi, s_log);
    }
    const double l0 = dmx_log_fast(G0 * cs.q0 + G1 * cs.q1 + G2 * cs.q2, s_log);                                  // llk0 (:459)
    v2d_t* o = reinterpret_cast<v2d_t*>(&s_ring[tile & 1u][w][lane][0]);
    v2d_t r01, r23;
    r01.x = t0; r01.y = t1; r23.x = t2; r23.y = l0;
    o[0] = r01; o[1] = r23;
    DMX_CP_BARRIER();
  };
  Hdr h1 = stage_b(stage_a(0));
  Hdr h2 = stage_b(stage_a(1));
  Raw pre = stage_a(2);
  Seed sA = stage_c(h1), sB = sA;
  for (uint32_t tile = 0; tile < ntiles; tile += 2) {
    {
      const Hdr cur = h1;
      h1 = h2;
      sB = stage_c(h1);                            // tile + 1
      h2 = stage_b(pre);                           // tile + 2
      pre = stage_a(tile + 3);                     // tile + 3
      compute(cur, sA, tile);
    }
    if (tile + 1 >= ntiles) break;
    {
      const Hdr cur = h1;
      h1 = h2;
      sA = stage_c(h1);
      h2 = stage_b(pre);
      pre = stage_a(tile + 4);
      compute(cur, sB, tile + 1);
    }
  }
}

// K1 over genotype classes, wide-panel form (V >= 20, measured crossover): all V+1 accumulators of a cell are summed in one pass per tile.
// Same walk and ownership as k_singlet; per pair the lane evaluates log(GL . row_d) once per class d plus the llk0 term,
// and stores those five terms and the SNP's packed class ids; chain lane (cell, k) then adds term[id[snp][k]] for the
// tile's pairs in ascending order — the very doubles k_singlet would have formed for sample k, in the same order.
// One barcode per wavefront (CW == 1).  L0M (panels of a multiple of 64 samples, cfg4's 64): the llk0 chain would be the ONLY chain of a second
// pass over the tile — a whole pass of index arithmetic and look-ups for one active lane, a third of the kernel's instructions at V = 64 — so
// it is merged into the first pass instead: every lane adds the tile's llk0 terms (uniform LDS reads) beside its own sample's, lane 0 stores.
template <int CW, int MINW = 4, bool L0M = false>
__global__ __launch_bounds__(kThreads, MINW) void k_singlet_clsw(PileupView pv, int nrd_width, const float* __restrict__ rows,
                                                             const uint32_t* __restrict__ idw, const double* __restrict__ gp0,
                                                             const double* __restrict__ tabs,
                                                             const int32_t* __restrict__ sched, int32_t V,
                                                             double* __restrict__ llks, double* __restrict__ llk0s) {
  constexpr int T = 64 / CW;
  constexpr int NW = kThreads / 64;
  constexpr int TD = 6;                          // doubles per pair in LDS: 4 class terms, llk0 term, 1 pad
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dynraw[];   // per wavefront: id words [nwd][64]
  __shared__ double s_tab[kTabK1];
  __shared__ __attribute__((aligned(16))) double s_term[NW][64 * TD];
  __shared__ __attribute__((aligned(16))) double s_t0[NW][64];      // L0M: the tile's llk0 terms, contiguous (the merged sum reads them two at a time)
  const double* s_log = s_tab + kLut;
  const double* s_first = s_tab + kTab;
  const double* s_final = s_first + kFirst;

  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int nwd = (V + 15) / 16;
  for (int i = t; i < kTabK1; i += kThreads) s_tab[i] = tabs[i];
  __syncthreads();                               // the only workgroup barrier

  double* term = s_term[w];
  double* t0s = s_t0[w];
  uint32_t* s_idw = reinterpret_cast<uint32_t*>(s_dynraw) + (size_t)w * 64 * nwd;
  const int slot0 = (blockIdx.x * NW + w) * CW;
  if (slot0 >= pv.B) return;

  const int c = lane / T, ti = lane % T;
  const bool cell_ok = slot0 + c < pv.B;
  const int32_t cell = cell_ok ? sched[slot0 + c] : 0;
  const int64_t p_beg = cell_ok ? pv.cell_pair_off[cell] : 0;
  const int64_t np = cell_ok ? pv.cell_pair_off[cell + 1] - p_beg : 0;
  int64_t rd_base = cell_ok ? pv.cell_read_off[cell] : 0;
  int64_t max_np = np;
#pragma unroll
  for (int d = T; d < 64; d <<= 1) max_np = max(max_np, __shfl_xor(max_np, d));

  // chains: a = lane + 64*i over the barcode's accumulators, sample a for a < V; a == V is llk0 unless it is merged (L0M).  A wavefront
  // carries 256 chains; wider panels are cut into chain slabs over blockIdx.y, each repeating the five logs per pair.
  static_assert(CW == 1, "one barcode per wavefront");
  constexpr int MAXCH = 4;
  const int nchain = L0M ? V : V + 1;
  double acc[MAXCH];
  [[maybe_unused]] double acc0 = 0.0;            // L0M: the llk0 sum, on every lane of chain slab 0
  int32_t ch_k[MAXCH];
#pragma unroll
  for (int i = 0; i < MAXCH; ++i) {
    const int a = (int)blockIdx.y * 64 * MAXCH + lane + 64 * i;
    acc[i] = 0.0;
    ch_k[i] = (cell_ok && a < nchain) ? a : -1;
  }
  const bool slab0 = blockIdx.y == 0;

  struct Raw { uint32_t n; int32_t snp; };
  struct Hdr { uint32_t n; int32_t snp; uint32_t rd4; int64_t off; };
  auto issue = [&](int64_t tile) {
    Raw r;
    const int64_t pi = tile * T + ti;
    const bool v = pi < np;
    r.n = v ? load_nrd(pv.pair_nrd, p_beg + pi, nrd_width) : 0u;
    r.snp = v ? (pv.pair_snp ? pv.pair_snp[p_beg + pi] : (int32_t)pi) : 0;
    return r;
  };
  auto prepare = [&](const Raw& r) {
    Hdr h;
    h.n = r.n; h.snp = r.snp;
    const uint32_t incl = seg_scan_incl<T>(r.n);
    h.off = rd_base + (int64_t)(incl - r.n);
    rd_base += seg_last<T>(incl, lane);
    h.rd4 = 0;
    if (r.n > 0) {
      if (h.off + 4 <= pv.R) __builtin_memcpy(&h.rd4, pv.reads + h.off, 4);
      else for (int64_t i = h.off; i < pv.R; ++i) h.rd4 |= (uint32_t)pv.reads[i] << (8 * (int)(i - h.off));
    }
    return h;
  };

  Hdr nxt = prepare(issue(0));
  Raw pre = issue(1);
  for (int64_t tile = 0; tile * T < max_np; ++tile) {
    const Hdr cur = nxt;
    nxt = prepare(pre);
    pre = issue(tile + 2);
    const bool valid = tile * T + ti < np;

    // class rows, llk0 row and id words of this lane's SNP (48 + 24 + 4*nwd bytes, SNP-major: contiguous across a dense tile)
    const float4* rp = reinterpret_cast<const float4*>(rows + (size_t)cur.snp * 12);
    const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2];
    const double* g0 = gp0 + (size_t)cur.snp * 3;
    const double q0 = g0[0], q1 = g0[1], q2 = g0[2];
    for (int wq = 0; wq < nwd; ++wq) s_idw[wq * 64 + lane] = idw[(size_t)cur.snp * nwd + wq];   // [word][pair]: a chain reads four pairs' words at once

    double G0, G1, G2;                                                       // :427-452, as in k_singlet
    {
      const uint32_t n = cur.n;
      const uint32_t b0 = cur.rd4 & 0xFFu;
      const double* f = s_final + 3 * (n ? b0 : 256u);
      G0 = f[0]; G1 = f[1]; G2 = f[2];
      if (n >= 2) {
        const double* f1 = s_first + 3 * b0;
        G0 = f1[0]; G1 = f1[1]; G2 = f1[2];
        gl_continue(1u, n, cur.rd4, pv.reads, cur.off, s_tab, G0, G1, G2);
      }
    }
    if (valid) {
      const double x0 = G0 * (double)r0.x + G1 * (double)r0.y + G2 * (double)r0.z;     // class 0   (:456)
      const double x1 = G0 * (double)r0.w + G1 * (double)r1.x + G2 * (double)r1.y;     // class 1
      const double x2 = G0 * (double)r1.z + G1 * (double)r1.w + G2 * (double)r2.x;     // class 2
      const double x3 = G0 * (double)r2.y + G1 * (double)r2.z + G2 * (double)r2.w;     // class 3
      const double x4 = G0 * q0 + G1 * q1 + G2 * q2;                                    // llk0      (:459)
      const bool fast_ok = __builtin_amdgcn_class(x0, 0x100) && __builtin_amdgcn_class(x1, 0x100) && __builtin_amdgcn_class(x2, 0x100) &&
                           __builtin_amdgcn_class(x3, 0x100) && __builtin_amdgcn_class(x4, 0x100);
      double* tr = &term[lane * TD];
      tr[0] = dmx_log_fast(x0, s_log); tr[1] = dmx_log_fast(x1, s_log); tr[2] = dmx_log_fast(x2, s_log);
      tr[3] = dmx_log_fast(x3, s_log); tr[4] = dmx_log_fast(x4, s_log);
      if (__builtin_expect(!fast_ok, 0)) {         // never for real likelihoods; keeps log(0) / log(nan) semantics
        const double xs[5] = {x0, x1, x2, x3, x4};
        for (int d = 0; d < 5; ++d) if (!__builtin_amdgcn_class(xs[d], 0x100)) tr[d] = log(xs[d]);
      }
      if (L0M) t0s[lane] = tr[4];
    }
    DMX_WAVE_LDS_ORDER();
    // ---- ordered sums: chain k adds term[pair][class of sample k at the pair's SNP] for the tile's pairs
    const int64_t left = np - tile * T;            // (np is the wavefront's one barcode's: uniform)
    const int cnt = left >= T ? T : (left > 0 ? (int)left : 0);
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
      const bool merged = L0M && i == 0 && slab0;  // this pass also carries the llk0 sum
      if (ch_k[i] < 0 && !merged) continue;
      const int k = ch_k[i] < 0 ? 0 : ch_k[i];     // (merged pass: lanes without a chain walk along with sample 0's look-ups, unused)
      const bool is0 = !L0M && k == V;             // (with L0M no chain is the llk0 chain: the test and its select compile away)
      const int wq = is0 ? 0 : (k >> 4), sh = is0 ? 0 : 2 * (k & 15);
      const double* tb = &term[0];
      const uint32_t* ib = &s_idw[wq * 64];
      // Round 5: the walk is instantiated with and without the merged llk0 sum (it used to test `merged` — a scalar branch — at every pair), the id
      // words of eight pairs come as two 16-byte reads from the transposed [word][pair] layout (they were eight reads through eight separately
      // advanced addresses): 10 -> 4 VALU instructions per (pair, chain) — extract, scale-and-add, the two adds.
      auto walk = [&](auto merged_c) {
        constexpr bool MG = decltype(merged_c)::value;
        double s = acc[i];
        int p = 0;
        constexpr int NB = L0M ? 8 : 16;           // pairs per batch: ids first, then the term reads, then the ordered adds
        for (; p + NB <= cnt; p += NB) {
          uint32_t wv[NB];
#pragma unroll
          for (int q4 = 0; q4 < NB / 4; ++q4) {
            const uint4 u = *reinterpret_cast<const uint4*>(&ib[p + 4 * q4]);
            wv[4 * q4] = u.x; wv[4 * q4 + 1] = u.y; wv[4 * q4 + 2] = u.z; wv[4 * q4 + 3] = u.w;
          }
          double tv[NB];
          [[maybe_unused]] double t0v[NB];
#pragma unroll
          for (int q = 0; q < NB; ++q) {
            const uint32_t d = is0 ? 4u : ((wv[q] >> sh) & 3u);
            tv[q] = tb[(p + q) * TD + d];
          }
          if (MG) {                                  // (uniform addresses; taking the terms from their pairs' lanes with v_readlane instead: 28.6 -> 34.1 ms)
#pragma unroll
            for (int q = 0; q < NB; q += 2) {
              const double2 u = *reinterpret_cast<const double2*>(&t0s[p + q]);
              t0v[q] = u.x; t0v[q + 1] = u.y;
            }
          }
#pragma unroll
          for (int q = 0; q < NB; ++q) {             // ascending SNP order: the reference's order
            s += tv[q];
            if (MG) acc0 += t0v[q];
          }
        }
        for (; p < cnt; ++p) {
          const uint32_t d = is0 ? 4u : ((ib[p] >> sh) & 3u);
          s += tb[p * TD + d];
          if (MG) acc0 += tb[p * TD + 4];
        }
        acc[i] = s;
      };
      if (merged) walk(std::true_type{}); else walk(std::false_type{});
    }
    DMX_WAVE_LDS_ORDER();
  }
#pragma unroll
  for (int i = 0; i < MAXCH; ++i) {
    if (ch_k[i] < 0) continue;
    if (ch_k[i] < V) llks[(size_t)cell * V + ch_k[i]] = acc[i];
    else llk0s[cell] = acc[i];
  }
  if (L0M && slab0 && cell_ok && lane == 0) llk0s[cell] = acc0;
}

// Where every cell stands at the boundaries of the SNP blocks [b << shift, (b + 1) << shift): blk[cell][b] = {index of its first
// pair with SNP id >= b << shift, first read byte of that pair}, b = 0..nblk (the last entry is the cell's end).  One wavefront per
// cell, one pass over its pair headers; built once per staged pileup (K1's blocked walk: sparse pileups; the genotype refinement: either
// layout — pair t of a dense pileup's cell is SNP t).
__global__ __launch_bounds__(kThreads) void k_snp_blocks(PileupView pv, int nrd_width, int shift, int32_t nblk, int64_t* __restrict__ blk) {
  const int lane = threadIdx.x & 63;
  const int32_t cell = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (cell >= pv.B) return;
  const int64_t p_beg = pv.cell_pair_off[cell], p_end = pv.cell_pair_off[cell + 1];
  int64_t rd_base = pv.cell_read_off[cell];
  int64_t* out = blk + (size_t)cell * (nblk + 1) * 2;
  int32_t b_prev = -1;                            // block of the last pair seen (wave-uniform)
  for (int64_t p0 = p_beg; p0 < p_end; p0 += 64) {
    const int64_t p = p0 + lane;
    const bool v = p < p_end;
    const uint32_t n = v ? load_nrd(pv.pair_nrd, p, nrd_width) : 0u;
    const int32_t b = v ? ((pv.pair_snp ? pv.pair_snp[p] : (int32_t)(p - p_beg)) >> shift) : 0x7FFFFFFF;
    const uint32_t incl = seg_scan_incl<64>(n);
    const int64_t off = rd_base + (int64_t)(incl - n);
    int32_t bp = __shfl_up(b, 1);
    if (lane == 0) bp = b_prev;
    if (v) for (int32_t bb = bp + 1; bb <= min(b, nblk); ++bb) { out[2 * bb] = p; out[2 * bb + 1] = off; }
    rd_base += (int64_t)__builtin_amdgcn_readlane((int)incl, 63);
    const int last = (int)min((int64_t)63, p_end - p0 - 1);
    b_prev = __shfl(b, last);
  }
  for (int32_t bb = b_prev + 1 + lane; bb <= nblk; bb += 64) { out[2 * bb] = p_end; out[2 * bb + 1] = rd_base; }
}

// ---- genotype refinement (dmx_engine_refine_genotypes) ----------------------------------------------------------
// LL[i][v][g] = sum of log(GL_{b,i}[g]) over the barcodes b assigned to sample v that have a pair at SNP i, with the pair counts and the
// stored reads of allele 0 / 1.  Sum order (the contract): a sample's assigned barcodes in ascending cell id, cut into chunks of
// kRefChunk; inside a chunk the terms are added in barcode order (k_refine_partial), then the chunk partials in ascending chunk order
// (k_refine_fold).  No floating-point atomics anywhere: the result does not depend on launch geometry, waves or what ran before.
constexpr int kRefChunk = 64;                    // C: assigned barcodes per chunk
constexpr int kRefSlabShift = 9, kRefSlab = 1 << kRefSlabShift;   // SNPs per slab: one workgroup's LDS accumulators
struct RefPartial { double ll[3]; int32_t n_cell, n_ref, n_alt, pad; };

// One wavefront per (chunk, SNP slab): the chunk's barcodes one after another; per barcode, the lanes take its pairs inside the slab
// (k_snp_blocks' table gives the first pair and read byte, so no barcode prefix is walked twice), a wavefront scan of pair_nrd gives
// the read offsets as in K1, the GL comes from K1's shared device path (gl_seed's tables, gl_finish's recurrence for deeper pairs) and
// each lane adds its three logs and counts into the slab's LDS accumulator of its SNP.  A barcode has at most one pair per SNP, so
// lanes never collide, and the LDS executes one wavefront's instructions in program order, so barcode b + 1 adds after barcode b.
__global__ __launch_bounds__(64) void k_refine_partial(PileupView pv, int nrd_width, const double* __restrict__ tabs, const int64_t* __restrict__ blk,
                                                       int32_t nblk, const int32_t* __restrict__ members, const int32_t* __restrict__ chunk_beg,
                                                       int32_t c0, RefPartial* __restrict__ partial) {
  __shared__ double s_log[DMX_LOG_TABLE_DOUBLES];
  __shared__ double s_ll[3][kRefSlab];
  __shared__ int32_t s_n[3][kRefSlab];
  const int lane = threadIdx.x;
  const int32_t slab = blockIdx.x, chunk = c0 + (int32_t)blockIdx.y;
  const int32_t s0 = slab << kRefSlabShift;
  for (int i = lane; i < DMX_LOG_TABLE_DOUBLES; i += 64) s_log[i] = tabs[kLut + i];
  for (int i = lane; i < kRefSlab; i += 64) {
#pragma unroll
    for (int g = 0; g < 3; ++g) { s_ll[g][i] = 0.0; s_n[g][i] = 0; }
  }
  __syncthreads();
  const DmxLogPins lk = dmx_log_pins();
  const int32_t m_end = chunk_beg[chunk + 1];
  for (int32_t m = chunk_beg[chunk]; m < m_end; ++m) {
    const int32_t cell = members[m];
    const int64_t* bt = blk + ((size_t)cell * (nblk + 1) + slab) * 2;
    const int64_t p_end = bt[2], cell_p0 = pv.cell_pair_off[cell];
    int64_t rd_base = bt[1];
    for (int64_t p0 = bt[0]; p0 < p_end; p0 += 64) {
      const int64_t p = p0 + lane;
      const bool v = p < p_end;
      const uint32_t n = v ? load_nrd(pv.pair_nrd, p, nrd_width) : 0u;
      const int32_t snp = v ? (pv.pair_snp ? pv.pair_snp[p] : (int32_t)(p - cell_p0)) : 0;
      const uint32_t incl = seg_scan_incl<64>(n);
      const int64_t off = rd_base + (int64_t)(incl - n);
      rd_base += (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      const int k = snp - s0;                          // inside the slab by construction (pairs in ascending SNP order); checked all the same
      if (v && (unsigned)k < (unsigned)kRefSlab) {
        const uint32_t rd4 = load_rd4(pv, off, n);
        const GlSeed sd = gl_seed(tabs, n, rd4);
        double G0, G1, G2;
        gl_finish(sd, n, rd4, pv.reads, off, tabs, G0, G1, G2);
        uint32_t alt = 0;
        for (uint32_t r = 0; r < n && r < 4; ++r) alt += (rd4 >> (8 * r + 7)) & 1u;
        for (uint32_t r = 4; r < n; ++r) alt += (uint32_t)pv.reads[off + r] >> 7;
        s_ll[0][k] += dmx_log_fast_pinned(G0, s_log, lk);    // GL >= 1e-6 / (1 + 3e-6): a normal positive argument
        s_ll[1][k] += dmx_log_fast_pinned(G1, s_log, lk);
        s_ll[2][k] += dmx_log_fast_pinned(G2, s_log, lk);
        s_n[0][k] += 1; s_n[1][k] += (int32_t)(n - alt); s_n[2][k] += (int32_t)alt;
      }
      DMX_WAVE_LDS_ORDER();
    }
  }
  RefPartial* out = partial + (size_t)blockIdx.y * pv.S + s0;
  const int lim = min(kRefSlab, pv.S - s0);
  for (int i = lane; i < lim; i += 64) {
    RefPartial r;
    r.ll[0] = s_ll[0][i]; r.ll[1] = s_ll[1][i]; r.ll[2] = s_ll[2][i];
    r.n_cell = s_n[0][i]; r.n_ref = s_n[1][i]; r.n_alt = s_n[2][i]; r.pad = 0;
    out[i] = r;
  }
}

// One lane per (SNP i, sample v), i fastest (the partial rows of a chunk are read contiguously): adds the sample's chunks [c0, c1) of this
// wave of partials, in ascending chunk order, onto the running sums (zeroed before the first wave).
__global__ __launch_bounds__(256) void k_refine_fold(const RefPartial* __restrict__ partial, int32_t S, int32_t V, const int32_t* __restrict__ samp_chunk,
                                                     int32_t c0, int32_t c1, double* __restrict__ ll, int32_t* __restrict__ cnt) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)S * V) return;
  const int32_t v = (int32_t)(t / S), i = (int32_t)(t % S);
  const int32_t cb = max(samp_chunk[v], c0), ce = min(samp_chunk[v + 1], c1);
  if (cb >= ce) return;
  const size_t o = (size_t)i * V + v, SV = (size_t)S * V;
  double a0 = ll[o * 3], a1 = ll[o * 3 + 1], a2 = ll[o * 3 + 2];
  int32_t n0 = cnt[o], n1 = cnt[SV + o], n2 = cnt[2 * SV + o];
  for (int32_t c = cb; c < ce; ++c) {
    const RefPartial& r = partial[(size_t)(c - c0) * S + i];
    a0 += r.ll[0]; a1 += r.ll[1]; a2 += r.ll[2];
    n0 += r.n_cell; n1 += r.n_ref; n2 += r.n_alt;
  }
  ll[o * 3] = a0; ll[o * 3 + 1] = a1; ll[o * 3 + 2] = a2;
  cnt[o] = n0; cnt[SV + o] = n1; cnt[2 * SV + o] = n2;
}

// gp'[i][v][g] = q[g] exp(LL[g] - max LL) / sum, q[g] = prior[i][v][g] + floor, in float64, rounded to float32; rows no pair covers keep the prior's bits.
__global__ __launch_bounds__(256) void k_refine_finish(const double* __restrict__ ll, const int32_t* __restrict__ n_cell, const float* __restrict__ prior,
                                                       int64_t n_rows, double floor_, float* __restrict__ gp) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_rows) return;
  if (n_cell[o] == 0) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(prior) + o * 3;
    uint32_t* dst = reinterpret_cast<uint32_t*>(gp) + o * 3;
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    return;
  }
  const double l0 = ll[o * 3], l1 = ll[o * 3 + 1], l2 = ll[o * 3 + 2];
  const double mx = fmax(fmax(l0, l1), l2);
  const double w0 = ((double)prior[o * 3] + floor_) * exp(l0 - mx);
  const double w1 = ((double)prior[o * 3 + 1] + floor_) * exp(l1 - mx);
  const double w2 = ((double)prior[o * 3 + 2] + floor_) * exp(l2 - mx);
  const double sum = w0 + w1 + w2;
  gp[o * 3] = (float)(w0 / sum); gp[o * 3 + 1] = (float)(w1 / sum); gp[o * 3 + 2] = (float)(w2 / sum);
}

// ---- genotype-free clustering (dmx_engine_cluster_*) ------------------------------------------------------------
// The stage writes, for every pair of the staged pileup, lgl[3] = log GL (the refinement's vector: gl_seed / gl_finish, then
// dmx_log_fast_pinned) and its stored REF / ALT reads (ref | alt << 16), in SNP-major order with ascending cell id inside a SNP, and the
// cell id of each slot.  One wavefront per cell walks its pairs as k_refine_partial does; `dst` maps a cell-major pair to its slot
// (NULL: the dense layout, slot = t * B + cell for pair t of the cell; else k_cluster_slots made it).
__global__ __launch_bounds__(kThreads) void k_cluster_lgl(PileupView pv, int nrd_width, const double* __restrict__ tabs, int64_t p_base,
                                                          const int32_t* __restrict__ dst, double* __restrict__ lgl, uint32_t* __restrict__ cnt,
                                                          int32_t* __restrict__ cell_of, int32_t* __restrict__ deep) {
  __shared__ double s_log[DMX_LOG_TABLE_DOUBLES];
  for (int i = threadIdx.x; i < DMX_LOG_TABLE_DOUBLES; i += blockDim.x) s_log[i] = tabs[kLut + i];
  __syncthreads();
  const DmxLogPins lk = dmx_log_pins();
  const int lane = threadIdx.x & 63;
  const int32_t cell = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (cell >= pv.B) return;
  const int64_t p_beg = pv.cell_pair_off[cell], p_end = pv.cell_pair_off[cell + 1];
  int64_t rd_base = pv.cell_read_off[cell];
  for (int64_t p0 = p_beg; p0 < p_end; p0 += 64) {
    const int64_t p = p0 + lane;
    const bool v = p < p_end;
    const uint32_t n = v ? load_nrd(pv.pair_nrd, p, nrd_width) : 0u;
    const uint32_t incl = seg_scan_incl<64>(n);
    const int64_t off = rd_base + (int64_t)(incl - n);
    rd_base += (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (v) {
      const uint32_t rd4 = load_rd4(pv, off, n);
      const GlSeed sd = gl_seed(tabs, n, rd4);
      double G0, G1, G2;
      gl_finish(sd, n, rd4, pv.reads, off, tabs, G0, G1, G2);
      uint32_t alt = 0;
      for (uint32_t r = 0; r < n && r < 4; ++r) alt += (rd4 >> (8 * r + 7)) & 1u;
      for (uint32_t r = 4; r < n; ++r) alt += (uint32_t)pv.reads[off + r] >> 7;
      const int64_t j = dst ? (int64_t)dst[p - p_base] : (p - p_beg) * (int64_t)pv.B + cell;
      lgl[3 * j] = dmx_log_fast_pinned(G0, s_log, lk);      // GL >= 1e-6 / (1 + 3e-6): a normal positive argument
      lgl[3 * j + 1] = dmx_log_fast_pinned(G1, s_log, lk);
      lgl[3 * j + 2] = dmx_log_fast_pinned(G2, s_log, lk);
      if (n > 0xFFFFu) *deep = 1;                           // the stage refuses pairs of more than 65 535 stored reads
      cnt[j] = (n - alt) | (alt << 16);
      cell_of[j] = cell;
    }
  }
}

// Sparse stage: the slot of a pair is snp_off[s] + (barcodes of lower id with a pair at s), computed without atomics.  The barcodes are
// cut into groups of `gsz`, the SNPs into slabs of kClSlab (k_snp_blocks' table gives each barcode's first pair in a slab); one
// wavefront per (slab, group) walks the group's barcodes in ascending id with LDS counters of the slab's SNPs — a barcode has at most
// one pair per SNP, so lanes never collide, and the LDS executes one wavefront's instructions in program order.
//   RANK = false: M[g][s] = the group's barcodes with a pair at s.
//   RANK = true:  the counters start at snp_off[s] + M[g][s] (k_cluster_colscan made M exclusive over the groups) and each pair takes
//                 the next slot: dst[p - p_base].
constexpr int kClSlabShift = 12, kClSlab = 1 << kClSlabShift;
template <bool RANK>
__global__ __launch_bounds__(64) void k_cluster_slots(PileupView pv, const int64_t* __restrict__ blk, int32_t nblk, int32_t gsz, int64_t p_base,
                                                      int32_t* __restrict__ M, const int64_t* __restrict__ snp_off, int32_t* __restrict__ dst) {
  __shared__ int32_t s_c[kClSlab];
  const int lane = threadIdx.x;
  const int32_t slab = blockIdx.x, g = blockIdx.y, S = pv.S;
  const int32_t s0 = slab << kClSlabShift, lim = min(kClSlab, S - s0);
  for (int i = lane; i < kClSlab; i += 64) s_c[i] = (RANK && i < lim) ? (int32_t)snp_off[s0 + i] + M[(size_t)g * S + s0 + i] : 0;
  __syncthreads();
  const int32_t c0 = g * gsz, c1 = min(pv.B, c0 + gsz);
  for (int32_t cell = c0; cell < c1; ++cell) {
    const int64_t* bt = blk + ((size_t)cell * (nblk + 1) + slab) * 2;
    const int64_t pe = bt[2];
    for (int64_t p0 = bt[0]; p0 < pe; p0 += 64) {
      const int64_t p = p0 + lane;
      const int32_t k = p < pe ? pv.pair_snp[p] - s0 : -1;
      if ((unsigned)k < (unsigned)lim) {
        if (RANK) dst[p - p_base] = s_c[k];
        s_c[k] += 1;
      }
      DMX_WAVE_LDS_ORDER();
    }
  }
  __syncthreads();
  if (!RANK) for (int i = lane; i < lim; i += 64) M[(size_t)g * S + s0 + i] = s_c[i];
}
// per SNP: M[g][s] -> its exclusive prefix over the groups, tot[s] = the SNP's pairs
__global__ __launch_bounds__(256) void k_cluster_colscan(int32_t* __restrict__ M, int32_t n_groups, int32_t S, int32_t* __restrict__ tot) {
  const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  int32_t a = 0;
  for (int32_t g = 0; g < n_groups; ++g) { const int32_t t = M[(size_t)g * S + s]; M[(size_t)g * S + s] = a; a += t; }
  tot[s] = a;
}

// M-step.  One wavefront per SNP i, one lane per column c (blockIdx.y selects 64 columns): over the SNP's slots in ascending cell id,
//   LL[i][c][g] = fma(w[b][c], lgl[g], LL) from 0,  W[i][c] += w[b][c];
// then gp'[i][c][g] = q[g] exp(LL[g] - max LL) / sum, q[g] = prior[i][g] + floor, in float64, rounded to float32; W = 0: prior's bits.
// The sum order is the contract (include/dmx.h): serial in slot order whatever the grid, no atomics.
__global__ __launch_bounds__(256) void k_cluster_mstep(const int64_t* __restrict__ snp_off, const int32_t* __restrict__ cell_of,
                                                       const double* __restrict__ lgl, const double* __restrict__ w, int32_t S, int32_t C,
                                                       const float* __restrict__ prior, double floor_, double* __restrict__ LL,
                                                       double* __restrict__ W, float* __restrict__ gp) {
  const int32_t i = __builtin_amdgcn_readfirstlane((int32_t)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (i >= S) return;
  const int32_t c = blockIdx.y * 64 + (threadIdx.x & 63);
  const bool on = c < C;
  const int32_t cc = on ? c : 0;
  const int64_t j0 = snp_off[i], j1 = snp_off[i + 1];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, ws = 0.0;
  int64_t j = j0;
  for (; j + 4 <= j1; j += 4) {
    double x[4], l[12];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = w[(size_t)cell_of[j + u] * C + cc];
#pragma unroll
    for (int u = 0; u < 12; ++u) l[u] = lgl[3 * j + u];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a0 = fma(x[u], l[3 * u], a0); a1 = fma(x[u], l[3 * u + 1], a1); a2 = fma(x[u], l[3 * u + 2], a2); ws += x[u];
    }
  }
  for (; j < j1; ++j) {
    const double x = w[(size_t)cell_of[j] * C + cc];
    a0 = fma(x, lgl[3 * j], a0); a1 = fma(x, lgl[3 * j + 1], a1); a2 = fma(x, lgl[3 * j + 2], a2); ws += x;
  }
  if (!on) return;
  const size_t o = (size_t)i * C + c;
  LL[3 * o] = a0; LL[3 * o + 1] = a1; LL[3 * o + 2] = a2; W[o] = ws;
  if (ws == 0.0) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(prior) + (size_t)i * 3;
    uint32_t* d = reinterpret_cast<uint32_t*>(gp) + 3 * o;
    d[0] = src[0]; d[1] = src[1]; d[2] = src[2];
    return;
  }
  const double mx = fmax(fmax(a0, a1), a2);
  const double w0 = ((double)prior[(size_t)i * 3] + floor_) * exp(a0 - mx);
  const double w1 = ((double)prior[(size_t)i * 3 + 1] + floor_) * exp(a1 - mx);
  const double w2 = ((double)prior[(size_t)i * 3 + 2] + floor_) * exp(a2 - mx);
  const double sum = w0 + w1 + w2;
  gp[3 * o] = (float)(w0 / sum); gp[3 * o + 1] = (float)(w1 / sum); gp[3 * o + 2] = (float)(w2 / sum);
}

// E-step.  One thread per (barcode b, restart r), columns rK .. rK + K - 1 of K1's llks[B][C]:
//   a_k = (llks[b][rK + k] + log_pi[r][k]) / T,  w[b][rK + k] = exp(a_k - max a) / sum;  lse[b][r] = logsumexp_k(llks + log_pi);
// a barcode outside the mask gets w = 0 and lse = 0.  The body is shared with the grouped E-step (k_cluster_estep_grp, section 16).
__device__ __forceinline__ void cluster_estep_one(const double* __restrict__ llks, int32_t b, int32_t r, int32_t R, int32_t K,
                                                  const double* __restrict__ log_pi, double inv_t, bool in, double* __restrict__ w,
                                                  double* __restrict__ lse) {
  const size_t C = (size_t)R * K, o = (size_t)b * C + (size_t)r * K;
  if (!in) {
    for (int32_t k = 0; k < K; ++k) w[o + k] = 0.0;
    lse[(size_t)b * R + r] = 0.0;
    return;
  }
  double m = -INFINITY, m1 = -INFINITY;
  for (int32_t k = 0; k < K; ++k) {
    const double x = llks[o + k] + log_pi[(size_t)r * K + k];
    m1 = fmax(m1, x); m = fmax(m, x * inv_t);
  }
  double s = 0.0, s1 = 0.0;
  for (int32_t k = 0; k < K; ++k) {
    const double x = llks[o + k] + log_pi[(size_t)r * K + k];
    const double e = exp(x * inv_t - m);
    w[o + k] = e; s += e; s1 += exp(x - m1);
  }
  const double y = 1.0 / s;
  for (int32_t k = 0; k < K; ++k) w[o + k] *= y;
  lse[(size_t)b * R + r] = m1 + log(s1);
}
__global__ __launch_bounds__(256) void k_cluster_estep(const double* __restrict__ llks, int32_t B, int32_t R, int32_t K, const double* __restrict__ log_pi,
                                                       double inv_t, const uint8_t* __restrict__ mask, double* __restrict__ w, double* __restrict__ lse) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)B * R) return;
  const int32_t b = (int32_t)(t / R), r = (int32_t)(t % R);
  cluster_estep_one(llks, b, r, R, K, log_pi, inv_t, !(mask && !mask[b]), w, lse);
}

// The E-step's sums in a fixed order: chunk partials over kEChunk consecutive barcodes (one thread per output column, serial over the
// chunk's barcodes), then k_cluster_efold adds the chunks in ascending order.  Columns 0 .. C-1: sum of w; C .. C+R-1: sum of lse;
// with dm (the doublet E-step) C+R .. C+2R-1: sum of the doublet mass dm[b][r].
constexpr int kEChunk = 256;
__global__ __launch_bounds__(256) void k_cluster_epart(const double* __restrict__ w, const double* __restrict__ lse, const double* __restrict__ dm,
                                                       int32_t B, int32_t C, int32_t R, double* __restrict__ part) {
  const int32_t col = blockIdx.x * blockDim.x + threadIdx.x, ch = blockIdx.y;
  const int32_t ncol = C + R + (dm ? R : 0);
  if (col >= ncol) return;
  const int32_t b0 = ch * kEChunk, b1 = min(B, b0 + kEChunk);
  const bool is_w = col < C;
  const double* src = is_w ? w + col : col < C + R ? lse + (col - C) : dm + (col - C - R);
  const size_t stride = is_w ? (size_t)C : (size_t)R;
  double a = 0.0;
  for (int32_t b = b0; b < b1; ++b) a += src[(size_t)b * stride];
  part[(size_t)ch * ncol + col] = a;
}
__global__ __launch_bounds__(256) void k_cluster_efold(const double* __restrict__ part, int32_t n_chunks, int32_t n_cols, double* __restrict__ out) {
  const int32_t col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= n_cols) return;
  double a = 0.0;
  for (int32_t ch = 0; ch < n_chunks; ++ch) a += part[(size_t)ch * n_cols + col];
  out[col] = a;
}

// ---- doublet-aware clustering (dmx_engine_cluster_doublet / _estep_doublet) ---------------------------------------
// LLD[b][r][p] for every barcode b, restart r and pair p = (k, l), k < l, of the restart's K columns (lexicographic; pairs[p] = k | l << 16):
//   the sum over b's pairs in stored (ascending SNP) order of log(sum over x, y of gp[i][rK + k][x] gp[i][rK + l][y] pG[x + y]),
// pG[s] the reference's per-pair doublet factors at alpha = 0.5 (cmd_cram_demuxlet.cpp:594-663): per stored read, pG[s] *= pR (1 - s/4)
// + pA s/4, then every pG divided by their maximum; then + 1e-6 and the same renormalisation.  Only these five products exist at
// alpha = 0.5 (the reference's nine entries repeat them bit for bit), and with the grid {0, 0.5} their maximum is the reference's.
// One wavefront per (barcode, block of 64 pair-columns of the R x P), one lane per pair-column.  The wavefront stages 64 pairs at a
// time in LDS, one per lane (its SNP and its five pG values: the reads walk is lane-parallel over pairs), then every lane steps through
// them with broadcast reads and adds its own term serially.  Nothing crosses lanes and there are no atomics, so a pair-column's bits
// depend only on its two genotype columns and the barcode's reads: not on R, the block it falls in, or what ran before.
// The first block of a barcode also writes lsc[b] = the sum over its pairs, in the same order, of log(pG[0] + pG[2] + pG[4]): pG[2x]
// is the singlet genotype x's factor on the doublet's max-normalised scale, so LLD - lsc is on K1's sum-normalised one (the E-step).
constexpr int kDblWaves = 4;                     // wavefronts per workgroup: four (barcode, column block) units share the LDS tables
struct DblPair { double pg[5]; int32_t snp; int32_t pad; };

__global__ __launch_bounds__(64 * kDblWaves) void k_cluster_dbl(PileupView pv, int nrd_width, const double* __restrict__ tabs, const float* __restrict__ g,
                                                              int32_t V, int32_t K, int32_t P, const uint32_t* __restrict__ pairs, int32_t n_cols,
                                                              int32_t n_cblk, int64_t n_units, double* __restrict__ lld, double* __restrict__ lsc) {
  __shared__ double s_log[DMX_LOG_TABLE_DOUBLES];
  __shared__ double s_pra[256][2];               // by read byte (allele << 7 | bq): {pR, pA}
  __shared__ DblPair s_hdr[kDblWaves][64];
  __shared__ double s_ls[kDblWaves][64];         // log(pG[0] + pG[2] + pG[4]) of the staged pairs (first block of a barcode only)
  for (int i = threadIdx.x; i < DMX_LOG_TABLE_DOUBLES; i += 64 * kDblWaves) s_log[i] = tabs[kLut + i];
  for (int i = threadIdx.x; i < 256; i += 64 * kDblWaves) {
    const double mat = tabs[i & 127], e3 = tabs[128 + (i & 127)];
    s_pra[i][0] = (i >> 7) ? e3 : mat;
    s_pra[i][1] = (i >> 7) ? mat : e3;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t unit = (int64_t)blockIdx.x * kDblWaves + wave;
  if (unit >= n_units) return;
  const int32_t cell = (int32_t)(unit / n_cblk), cb = __builtin_amdgcn_readfirstlane((int32_t)(unit % n_cblk));
  double* ls = s_ls[wave];
  const int32_t c = cb * 64 + lane;
  const bool on = c < n_cols;                    // lanes past the last column run along with column 0 and write nothing
  const int32_t cc = on ? c : 0;
  const int32_t r = cc / P, kl = (int32_t)pairs[cc - r * P];
  const size_t ck = (size_t)(r * K + (kl & 0xFFFF)) * 3, cl = (size_t)(r * K + (kl >> 16)) * 3;
  const size_t row = (size_t)V * 3;
  DblPair* hdr = s_hdr[wave];
  const DmxLogPins lk = dmx_log_pins();
  const double wA[5] = {0.0, 0.25, 0.5, 0.75, 1.0}, wR[5] = {1.0, 0.75, 0.5, 0.25, 0.0};
  double acc = 0.0, acc_s = 0.0;
  const int64_t p_beg = pv.cell_pair_off[cell], p_end = pv.cell_pair_off[cell + 1];
  int64_t rd_base = pv.cell_read_off[cell];
  for (int64_t p0 = p_beg; p0 < p_end; p0 += 64) {
    const int64_t p = p0 + lane;
    const bool in = p < p_end;
    const uint32_t n = in ? load_nrd(pv.pair_nrd, p, nrd_width) : 0u;
    const uint32_t incl = seg_scan_incl<64>(n);
    const int64_t off = rd_base + (int64_t)(incl - n);
    rd_base += (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (in) {
      double pg[5] = {1.0, 1.0, 1.0, 1.0, 1.0};
      uint32_t w = load_rd4(pv, off, n);
      for (uint32_t t = 0; t < n; ++t) {
        if (t > 0 && (t & 3) == 0) w = load_rd4(pv, off + t, n - t);
        const uint32_t byte = (w >> (8 * (t & 3))) & 0xFF;
        const double pR = s_pra[byte][0], pA = s_pra[byte][1];
        double mx = 0.0;
#pragma unroll
        for (int s = 0; s < 5; ++s) { pg[s] *= pR * wR[s] + pA * wA[s]; mx = fmax(mx, pg[s]); }
#pragma unroll
        for (int s = 0; s < 5; ++s) pg[s] /= mx;
      }
      double mx = 0.0;
#pragma unroll
      for (int s = 0; s < 5; ++s) { pg[s] += 1e-6; mx = fmax(mx, pg[s]); }
      DblPair h;
#pragma unroll
      for (int s = 0; s < 5; ++s) h.pg[s] = pg[s] / mx;
      if (cb == 0) ls[lane] = log(h.pg[0] + h.pg[2] + h.pg[4]);
      h.snp = pv.pair_snp ? pv.pair_snp[p] : (int32_t)(p - p_beg);
      h.pad = 0;
      hdr[lane] = h;
    }
    DMX_WAVE_LDS_ORDER();
    const int cnt = (int)min<int64_t>(64, p_end - p0);
    if (cb == 0) for (int j = 0; j < cnt; ++j) acc_s += ls[j];
    for (int j = 0; j < cnt; ++j) {
      const int32_t snp = __builtin_amdgcn_readfirstlane(hdr[j].snp);
      const double q0 = hdr[j].pg[0], q1 = hdr[j].pg[1], q2 = hdr[j].pg[2], q3 = hdr[j].pg[3], q4 = hdr[j].pg[4];
      const float* gr = g + (size_t)snp * row;
      const double a0 = gr[ck], a1 = gr[ck + 1], a2 = gr[ck + 2];
      const double b0 = gr[cl], b1 = gr[cl + 1], b2 = gr[cl + 2];
      // sum over x of a_x (sum over y of b_y pG[x + y])
      const double t0 = __builtin_fma(b2, q2, __builtin_fma(b1, q1, b0 * q0));
      const double t1 = __builtin_fma(b2, q3, __builtin_fma(b1, q2, b0 * q1));
      const double t2 = __builtin_fma(b2, q4, __builtin_fma(b1, q3, b0 * q2));
      const double L = __builtin_fma(a2, t2, __builtin_fma(a1, t1, a0 * t0));
      acc += dmx_log_is_special(L) ? log(L) : dmx_log_fast_pinned(L, s_log, lk);
    }
    DMX_WAVE_LDS_ORDER();
  }
  if (on) lld[(size_t)cell * n_cols + c] = acc;
  if (cb == 0 && lane == 0) lsc[cell] = acc_s;
}

// Doublet E-step.  One thread per (barcode b, restart r): K singlet components with scores a_k = (llks[b][rK + k] + lps[r][k]) / T and
// P doublet components with d_p = (lld[b][r][p] - lsc[b] + lpd[r][p]) / T (the host made the log priors: lps = log(1 - delta) + log pi,
// lpd = log delta + log(2 pi_k pi_l / (1 - sum pi^2))).  w[b][rK + k] = exp(a_k - M) / Z, dm[b][r] = sum_p exp(d_p - M) / Z
// (M the maximum, Z the sum over all K + P), lse[b][r] = logsumexp over all K + P of the unscaled scores.  A barcode outside the
// mask gets w = 0, dm = 0 and lse = 0.  With every lpd = -inf this is k_cluster_estep's arithmetic, bit for bit.
__global__ __launch_bounds__(256) void k_cluster_estep_dbl(const double* __restrict__ llks, const double* __restrict__ lld,
                                                           const double* __restrict__ lsc, int32_t B, int32_t R,
                                                           int32_t K, int32_t P, const double* __restrict__ lps, const double* __restrict__ lpd,
                                                           double inv_t, const uint8_t* __restrict__ mask, double* __restrict__ w,
                                                           double* __restrict__ lse, double* __restrict__ dm) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)B * R) return;
  const int32_t b = (int32_t)(t / R), r = (int32_t)(t % R);
  const size_t C = (size_t)R * K, o = (size_t)b * C + (size_t)r * K;
  const double* ld = lld + ((size_t)b * R + r) * P;
  const double* pd = lpd + (size_t)r * P;
  const double sc = lsc[b];
  if (mask && !mask[b]) {
    for (int32_t k = 0; k < K; ++k) w[o + k] = 0.0;
    lse[(size_t)b * R + r] = 0.0;
    dm[(size_t)b * R + r] = 0.0;
    return;
  }
  double m = -INFINITY, m1 = -INFINITY;
  for (int32_t k = 0; k < K; ++k) {
    const double x = llks[o + k] + lps[(size_t)r * K + k];
    m1 = fmax(m1, x); m = fmax(m, x * inv_t);
  }
  for (int32_t p = 0; p < P; ++p) {
    const double x = (ld[p] - sc) + pd[p];
    m1 = fmax(m1, x); m = fmax(m, x * inv_t);
  }
  double s = 0.0, s1 = 0.0, sd = 0.0;
  for (int32_t k = 0; k < K; ++k) {
    const double x = llks[o + k] + lps[(size_t)r * K + k];
    const double e = exp(x * inv_t - m);
    w[o + k] = e; s += e; s1 += exp(x - m1);
  }
  for (int32_t p = 0; p < P; ++p) {
    const double x = (ld[p] - sc) + pd[p];
    const double e = exp(x * inv_t - m);
    sd += e; s1 += exp(x - m1);
  }
  s += sd;
  const double y = 1.0 / s;
  for (int32_t k = 0; k < K; ++k) w[o + k] *= y;
  dm[(size_t)b * R + r] = sd * y;
  lse[(size_t)b * R + r] = m1 + log(s1);
}

// ---- split-merge moves (dmx_engine_cluster_merge_score / _estep_grouped) ------------------------------------------
// The M-step's own genotype prior at SNP i: log pi[g] = log((q[i][g] + floor) / sum over g of (q + floor)), and a three-term logsumexp.
// One definition for the marginal and the pair kernels, so that the two read the same bits.
__device__ __forceinline__ void sm_log_prior(const float* __restrict__ q, double floor_, int32_t i, double lp[3]) {
  const double a0 = (double)q[(size_t)i * 3] + floor_, a1 = (double)q[(size_t)i * 3 + 1] + floor_, a2 = (double)q[(size_t)i * 3 + 2] + floor_;
  const double s = a0 + a1 + a2;
  lp[0] = log(a0 / s); lp[1] = log(a1 / s); lp[2] = log(a2 / s);
}
__device__ __forceinline__ double sm_lse3(double x0, double x1, double x2) {
  const double m = fmax(fmax(x0, x1), x2);
  return m + log(exp(x0 - m) + exp(x1 - m) + exp(x2 - m));
}

// The per-column marginal of the last M-step: one thread per (SNP i, column c) of its C columns,
//   A[i][c] = lse_g(log pi[i][g] + LL[i][c][g]),  F[i][c] = (W[i][c] > 0).
__global__ __launch_bounds__(256) void k_cluster_marg(const double* __restrict__ LL, const double* __restrict__ W, const float* __restrict__ q,
                                                      double floor_, int32_t S, int32_t C, double* __restrict__ A, uint8_t* __restrict__ F) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)S * C) return;
  const int32_t i = (int32_t)(t / C);
  double lp[3];
  sm_log_prior(q, floor_, i, lp);
  A[t] = sm_lse3(lp[0] + LL[3 * t], lp[1] + LL[3 * t + 1], lp[2] + LL[3 * t + 2]);
  F[t] = W[t] > 0.0 ? 1 : 0;
}

// Merge scores, partial over one chunk of kSmChunk SNPs: one workgroup per (chunk, restart r); thread t owns the pairs t, t + 256, ...
// (p = (k, l), k < l, lexicographic; P <= 2016 for K <= 64, so at most kSmPairs per thread).  The chunk's K LL rows, A values, flags and
// log priors go through LDS kSmStage SNPs at a time.  Per pair, over the SNPs in ascending order where both flags are set:
//   acc += (lse_g(log pi[g] + LL[i][rK + k][g] + LL[i][rK + l][g]) - A[i][rK + k]) - A[i][rK + l],  n += 1,
// serially from 0.  The chunk size is part of the contract (k_cluster_merge_fold adds the chunks in ascending order); a pair's bits
// depend on its two columns' values only: not on the grid, R, the restart's position in the engine or what ran before.
constexpr int kSmChunk = 256, kSmStage = 16, kSmMaxK = 64, kSmPairs = 8;
__global__ __launch_bounds__(256) void k_cluster_merge_part(const double* __restrict__ LL, const double* __restrict__ A, const uint8_t* __restrict__ F,
                                                            const float* __restrict__ q, double floor_, int32_t S, int32_t C, int32_t K, int32_t P,
                                                            double* __restrict__ part, int32_t* __restrict__ npart) {
  __shared__ double sLL[kSmStage][3 * kSmMaxK];
  __shared__ double sA[kSmStage][kSmMaxK];
  __shared__ double sLp[kSmStage][3];
  __shared__ uint8_t sF[kSmStage][kSmMaxK];
  const int32_t ch = blockIdx.x, r = blockIdx.y, nch = gridDim.x;
  int32_t pk[kSmPairs], pl[kSmPairs];
  bool act[kSmPairs];
#pragma unroll
  for (int u = 0; u < kSmPairs; ++u) {
    int32_t rem = (int32_t)threadIdx.x + 256 * u, k = 0;
    act[u] = rem < P;
    if (!act[u]) rem = 0;                                    // inactive slot: skipped below, never written
    while (rem >= K - 1 - k) { rem -= K - 1 - k; ++k; }
    pk[u] = k; pl[u] = k + 1 + rem;
  }
  double acc[kSmPairs];
  int32_t cnt[kSmPairs];
#pragma unroll
  for (int u = 0; u < kSmPairs; ++u) { acc[u] = 0.0; cnt[u] = 0; }
  const int32_t i0 = ch * kSmChunk, i1 = min(S, i0 + kSmChunk);
  const size_t c0 = (size_t)r * K;
  for (int32_t s0 = i0; s0 < i1; s0 += kSmStage) {
    const int32_t n = min(kSmStage, i1 - s0);
    __syncthreads();
    for (int32_t x = threadIdx.x; x < n * K; x += blockDim.x) {
      const int32_t j = x / K, c = x - j * K;
      const size_t o = (size_t)(s0 + j) * C + c0 + c;
      sLL[j][3 * c] = LL[3 * o]; sLL[j][3 * c + 1] = LL[3 * o + 1]; sLL[j][3 * c + 2] = LL[3 * o + 2];
      sA[j][c] = A[o]; sF[j][c] = F[o];
    }
    if ((int32_t)threadIdx.x < n) sm_log_prior(q, floor_, s0 + threadIdx.x, sLp[threadIdx.x]);
    __syncthreads();
    for (int32_t j = 0; j < n; ++j) {
#pragma unroll
      for (int u = 0; u < kSmPairs; ++u) {
        const int32_t k = pk[u], l = pl[u];
        if (act[u] && sF[j][k] && sF[j][l]) {
          const double t = sm_lse3(sLp[j][0] + sLL[j][3 * k] + sLL[j][3 * l], sLp[j][1] + sLL[j][3 * k + 1] + sLL[j][3 * l + 1],
                                   sLp[j][2] + sLL[j][3 * k + 2] + sLL[j][3 * l + 2]);
          acc[u] += (t - sA[j][k]) - sA[j][l];
          cnt[u] += 1;
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kSmPairs; ++u) {
    const int32_t p = (int32_t)threadIdx.x + 256 * u;
    if (p < P) {
      const size_t o = ((size_t)r * nch + ch) * P + p;
      part[o] = acc[u]; npart[o] = cnt[u];
    }
  }
}
// One thread per (restart, pair): the chunks in ascending order.
__global__ __launch_bounds__(256) void k_cluster_merge_fold(const double* __restrict__ part, const int32_t* __restrict__ npart, int32_t n_chunks,
                                                            int32_t R, int32_t P, double* __restrict__ bf, int32_t* __restrict__ nsh) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)R * P) return;
  const int32_t r = (int32_t)(t / P), p = (int32_t)(t % P);
  double a = 0.0;
  int32_t n = 0;
  for (int32_t ch = 0; ch < n_chunks; ++ch) {
    const size_t o = ((size_t)r * n_chunks + ch) * P + p;
    a += part[o]; n += npart[o];
  }
  bf[t] = a; nsh[t] = n;
}

// Grouped E-step: k_cluster_estep's arithmetic (cluster_estep_one), but restart r sees only the barcodes with group[b] == r / rpg (and in
// the mask); every other barcode gets w = 0 and lse = 0 in that restart.
__global__ __launch_bounds__(256) void k_cluster_estep_grp(const double* __restrict__ llks, int32_t B, int32_t R, int32_t K, const double* __restrict__ log_pi,
                                                           double inv_t, const uint8_t* __restrict__ mask, const int32_t* __restrict__ group, int32_t rpg,
                                                           double* __restrict__ w, double* __restrict__ lse) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)B * R) return;
  const int32_t b = (int32_t)(t / R), r = (int32_t)(t % R);
  cluster_estep_one(llks, b, r, R, K, log_pi, inv_t, (!mask || mask[b]) && group[b] == r / rpg, w, lse);
}

// ---- choosing the number of clusters (dmx_engine_cluster_evidence / _hard / _merge_columns) ---------------------
// Evidence of every column of the last M-step from k_cluster_marg's A[S][C] and flags F[S][C]: one thread per (chunk of kSmChunk SNPs,
// column c) adds A[i][c] of the SNPs with F[i][c] set, serially from 0 in ascending order, and counts them; k_cluster_ev_fold then adds
// the chunks in ascending order.  The chunk size is the merge score's, and part of the contract.  A column's bits depend on its own
// LL and W only: not on the grid, R, the column's position or what ran before.  A SNP with W = 0 is skipped, not added as a zero.
__global__ __launch_bounds__(256) void k_cluster_ev_part(const double* __restrict__ A, const uint8_t* __restrict__ F, int32_t S, int32_t C,
                                                         double* __restrict__ part, int32_t* __restrict__ npart) {
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x, ch = blockIdx.y;
  if (c >= C) return;
  const int32_t i0 = ch * kSmChunk, i1 = min(S, i0 + kSmChunk);
  double acc = 0.0;
  int32_t n = 0;
  for (int32_t i = i0; i < i1; ++i) {
    const size_t o = (size_t)i * C + c;
    if (F[o]) { acc += A[o]; n += 1; }
  }
  part[(size_t)ch * C + c] = acc; npart[(size_t)ch * C + c] = n;
}
__global__ __launch_bounds__(256) void k_cluster_ev_fold(const double* __restrict__ part, const int32_t* __restrict__ npart, int32_t n_chunks, int32_t C,
                                                         double* __restrict__ ev, int32_t* __restrict__ ncov) {
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double a = 0.0;
  int32_t n = 0;
  for (int32_t ch = 0; ch < n_chunks; ++ch) { a += part[(size_t)ch * C + c]; n += npart[(size_t)ch * C + c]; }
  ev[c] = a; ncov[c] = n;
}

// Hard labels.  One thread per (barcode b, restart r) over the E-step's weights w[B][R K], the active flags act[R K] and, with dm (the
// doublet E-step's mass [B][R]), LLD[B][R][P]:
//   outside the mask                label = -1
//   dm != NULL and dm[b][r] >= 0.5  label = -2 - p, p the pair (k, l), both active, of the highest LLD[b][r][p] (the lowest p on a tie);
//                                   dsc[b][r] = that LLD
//   otherwise                       label = the active k of the highest w[b][rK + k] (the lowest k on a tie)
// dsc is 0.0 unless the label is a doublet's.  hot[b][rK + k] = 1.0 at a singlet label's column, else 0.0: every entry of the row is
// written, and w is only read.  The host has checked that every restart has an active column (with dm: an active pair).
__global__ __launch_bounds__(256) void k_cluster_hard(const double* __restrict__ w, const double* __restrict__ dm, const double* __restrict__ lld,
                                                      const uint8_t* __restrict__ act, const uint8_t* __restrict__ mask, int32_t B, int32_t R, int32_t K,
                                                      int32_t P, int32_t* __restrict__ label, double* __restrict__ dsc, double* __restrict__ hot) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)B * R) return;
  const int32_t b = (int32_t)(t / R), r = (int32_t)(t % R);
  const size_t o = (size_t)b * R * K + (size_t)r * K;
  const uint8_t* a = act + (size_t)r * K;
  int32_t lab = -1;
  double sc = 0.0;
  if (!(mask && !mask[b])) {
    if (dm && dm[t] >= 0.5) {
      const double* ld = lld + (size_t)t * P;
      int32_t best = -1, p = 0;
      for (int32_t k = 0; k < K; ++k)
        for (int32_t l = k + 1; l < K; ++l, ++p)
          if (a[k] && a[l] && (best < 0 || ld[p] > sc)) { best = p; sc = ld[p]; }
      lab = -2 - best;
    } else {
      double top = 0.0;
      for (int32_t k = 0; k < K; ++k)
        if (a[k] && (lab < 0 || w[o + k] > top)) { lab = k; top = w[o + k]; }
    }
  }
  label[t] = lab; dsc[t] = sc;
  for (int32_t k = 0; k < K; ++k) hot[o + k] = k == lab ? 1.0 : 0.0;
}

// The hard labels' sums in the E-step's order: chunk partials over kEChunk consecutive barcodes (one thread per output column, serial
// over the chunk's barcodes), then k_cluster_hard_fold adds the chunks in ascending order.  Columns 0 .. C-1: barcodes labelled k of
// restart r (c = rK + k); C .. C+R-1: doublet-labelled barcodes of restart r, whose doublet scores go to dpart[ch][r] beside them.
__global__ __launch_bounds__(256) void k_cluster_hard_part(const int32_t* __restrict__ label, const double* __restrict__ dsc, int32_t B, int32_t R, int32_t K,
                                                           int32_t* __restrict__ ipart, double* __restrict__ dpart) {
  const int32_t col = blockIdx.x * blockDim.x + threadIdx.x, ch = blockIdx.y;
  const int32_t C = R * K, ncol = C + R;
  if (col >= ncol) return;
  const int32_t b0 = ch * kEChunk, b1 = min(B, b0 + kEChunk);
  int32_t n = 0;
  if (col < C) {
    const int32_t r = col / K, k = col - r * K;
    for (int32_t b = b0; b < b1; ++b) n += label[(size_t)b * R + r] == k;
  } else {
    const int32_t r = col - C;
    double acc = 0.0;
    for (int32_t b = b0; b < b1; ++b)
      if (label[(size_t)b * R + r] <= -2) { acc += dsc[(size_t)b * R + r]; n += 1; }
    dpart[(size_t)ch * R + r] = acc;
  }
  ipart[(size_t)ch * ncol + col] = n;
}
__global__ __launch_bounds__(256) void k_cluster_hard_fold(const int32_t* __restrict__ ipart, const double* __restrict__ dpart, int32_t n_chunks, int32_t C,
                                                           int32_t R, int32_t* __restrict__ iout, double* __restrict__ dout) {
  const int32_t col = blockIdx.x * blockDim.x + threadIdx.x, ncol = C + R;
  if (col >= ncol) return;
  int32_t n = 0;
  for (int32_t ch = 0; ch < n_chunks; ++ch) n += ipart[(size_t)ch * ncol + col];
  iout[col] = n;
  if (col >= C) {
    double a = 0.0;
    for (int32_t ch = 0; ch < n_chunks; ++ch) a += dpart[(size_t)ch * R + (col - C)];
    dout[col - C] = a;
  }
}

// Column merge, in place on the E-step's weights: one thread per (barcode b, restart r) with fi[r] = from >= 0 and fi[R + r] = into:
//   w[b][rK + into] = w[b][rK + into] + w[b][rK + from] (one addition), then w[b][rK + from] = 0.0.
__global__ __launch_bounds__(256) void k_cluster_merge_cols(double* __restrict__ w, const int32_t* __restrict__ fi, int32_t B, int32_t R, int32_t K) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)B * R) return;
  const int32_t b = (int32_t)(t / R), r = (int32_t)(t % R);
  const int32_t from = fi[r], into = fi[R + r];
  if (from < 0) return;
  const size_t o = (size_t)b * R * K + (size_t)r * K;
  w[o + into] = w[o + into] + w[o + from];
  w[o + from] = 0.0;
}

// ---- partly genotyped pools (dmx_engine_cluster_estep_known / _mstep_window) ------------------------------------
// The engine's V = Vk + R M columns are [Vk known donors | restart 0's M free columns | ... | restart R-1's M], the known ones shared
// by every restart.  E-step: one thread per (barcode b, restart r) over its Vk + M components, component k's llk at column
//   k < Vk: k,  k >= Vk: Vk + r M + (k - Vk);   a_k = (llks[b][col] + log_pi[r][k]) / T,  w = exp(a_k - max a) / sum,
// lse[b][r] = logsumexp_k(llks + log_pi); a barcode outside the mask gets w = 0 and lse = 0.  The operations, and their order, are
// cluster_estep_one's, so with Vk = 0 the results are k_cluster_estep's bit for bit.  wk[b][r][k] holds every component's weight (for
// the ordered column sums), wf[b][r M + m] the free ones (for the windowed M-step).
__device__ __forceinline__ int64_t known_llk_col(int32_t k, int32_t r, int32_t Vk, int32_t M) {
  return k < Vk ? (int64_t)k : (int64_t)Vk + (int64_t)r * M + (k - Vk);
}
__global__ __launch_bounds__(256) void k_cluster_estep_known(const double* __restrict__ llks, int32_t B, int32_t R, int32_t Vk, int32_t M,
                                                             const double* __restrict__ log_pi, double inv_t, const uint8_t* __restrict__ mask,
                                                             double* __restrict__ wk, double* __restrict__ wf, double* __restrict__ lse) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)B * R) return;
  const int32_t b = (int32_t)(t / R), r = (int32_t)(t % R), K = Vk + M;
  const size_t V = (size_t)Vk + (size_t)R * M, lo = (size_t)b * V, ko = ((size_t)b * R + r) * K, fo = (size_t)b * R * M + (size_t)r * M;
  const double* lp = log_pi + (size_t)r * K;
  if (mask && !mask[b]) {
    for (int32_t k = 0; k < K; ++k) wk[ko + k] = 0.0;
    for (int32_t k = 0; k < M; ++k) wf[fo + k] = 0.0;
    lse[(size_t)b * R + r] = 0.0;
    return;
  }
  double m = -INFINITY, m1 = -INFINITY;
  for (int32_t k = 0; k < K; ++k) {
    const double x = llks[lo + known_llk_col(k, r, Vk, M)] + lp[k];
    m1 = fmax(m1, x); m = fmax(m, x * inv_t);
  }
  double s = 0.0, s1 = 0.0;
  for (int32_t k = 0; k < K; ++k) {
    const double x = llks[lo + known_llk_col(k, r, Vk, M)] + lp[k];
    const double e = exp(x * inv_t - m);
    wk[ko + k] = e; s += e; s1 += exp(x - m1);
  }
  const double y = 1.0 / s;
  for (int32_t k = 0; k < K; ++k) {
    const double v = wk[ko + k] * y;
    wk[ko + k] = v;
    if (k >= Vk) wf[fo + (k - Vk)] = v;
  }
  lse[(size_t)b * R + r] = m1 + log(s1);
}

// Windowed M-step: k_cluster_mstep's arithmetic and sum order over the C = R M free columns only (w[B][C], LL[S][C][3], W[S][C]); gp'
// goes to columns Vk .. V-1 of gp[S][V][3] (the known columns are copied in by the caller).  With Vk = 0 every address and every
// operation is k_cluster_mstep's, so the bits are.
__global__ __launch_bounds__(256) void k_cluster_mstep_win(const int64_t* __restrict__ snp_off, const int32_t* __restrict__ cell_of,
                                                           const double* __restrict__ lgl, const double* __restrict__ w, int32_t S, int32_t C,
                                                           const float* __restrict__ prior, double floor_, double* __restrict__ LL,
                                                           double* __restrict__ W, float* __restrict__ gp, int32_t Vk) {
  const int32_t i = __builtin_amdgcn_readfirstlane((int32_t)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (i >= S) return;
  const int32_t c = blockIdx.y * 64 + (threadIdx.x & 63);
  const bool on = c < C;
  const int32_t cc = on ? c : 0;
  const int64_t j0 = snp_off[i], j1 = snp_off[i + 1];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, ws = 0.0;
  int64_t j = j0;
  for (; j + 4 <= j1; j += 4) {
    double x[4], l[12];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = w[(size_t)cell_of[j + u] * C + cc];
#pragma unroll
    for (int u = 0; u < 12; ++u) l[u] = lgl[3 * j + u];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a0 = fma(x[u], l[3 * u], a0); a1 = fma(x[u], l[3 * u + 1], a1); a2 = fma(x[u], l[3 * u + 2], a2); ws += x[u];
    }
  }
  for (; j < j1; ++j) {
    const double x = w[(size_t)cell_of[j] * C + cc];
    a0 = fma(x, lgl[3 * j], a0); a1 = fma(x, lgl[3 * j + 1], a1); a2 = fma(x, lgl[3 * j + 2], a2); ws += x;
  }
  if (!on) return;
  const size_t o = (size_t)i * C + c, og = (size_t)i * ((size_t)C + Vk) + Vk + c;
  LL[3 * o] = a0; LL[3 * o + 1] = a1; LL[3 * o + 2] = a2; W[o] = ws;
  if (ws == 0.0) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(prior) + (size_t)i * 3;
    uint32_t* d = reinterpret_cast<uint32_t*>(gp) + 3 * og;
    d[0] = src[0]; d[1] = src[1]; d[2] = src[2];
    return;
  }
  const double mx = fmax(fmax(a0, a1), a2);
  const double w0 = ((double)prior[(size_t)i * 3] + floor_) * exp(a0 - mx);
  const double w1 = ((double)prior[(size_t)i * 3 + 1] + floor_) * exp(a1 - mx);
  const double w2 = ((double)prior[(size_t)i * 3 + 2] + floor_) * exp(a2 - mx);
  const double sum = w0 + w1 + w2;
  gp[3 * og] = (float)(w0 / sum); gp[3 * og + 1] = (float)(w1 / sum); gp[3 * og + 2] = (float)(w2 / sum);
}

// ---- ambient contamination profile (dmx_engine_ambient) ---------------------------------------------------------
// For a barcode b assigned to sample v and a grid point rho: LL_b(rho) = sum over b's pairs, in stored (ascending SNP) order, of
// log(gp[i][v][0] f_0 + gp[i][v][1] f_1 + gp[i][v][2] f_2), f_g = product over the pair's stored reads of pR (1 - p_g) + pA p_g,
// p_g = (1 - rho) g / 2 + rho a_i.  One wavefront per (barcode, block of 64 grid points), one lane per grid point: every lane walks
// the same pairs and sums its own LL serially, so nothing crosses lanes and the bits depend only on the lane's rho.  The wavefront
// stages 64 pair headers at a time (read count, read offset by a DPP scan, first four read bytes, a_i, the gp row as float64) in
// LDS, then steps through them with broadcast reads.  f_g is rescaled by an exact power of two, 2^-e with e the exponent of
// max f_g over the genotypes with gp != 0, whenever that maximum falls below 2^-300 (checked every 8 reads; one read scales it by
// >= 2^-44 with PhredHelper's tables); the exponents add up in E and LL gets log(L) + E ln 2.  A term that falls out of range
// below that maximum is smaller than 2^-925 of L.
constexpr int kAmbWaves = 4;                     // wavefronts per workgroup: four (barcode, grid block) units share the LDS tables
constexpr double kAmbRescaleBelow = 0x1p-300;
struct AmbPair { double a, g0, g1, g2; int64_t off; uint32_t n, rd4; };    // n = 0: the pair does not contribute

__global__ __launch_bounds__(64 * kAmbWaves) void k_ambient(PileupView pv, int nrd_width, const double* __restrict__ tabs, const float* __restrict__ g,
                                                          int32_t V, const int32_t* __restrict__ assign, const double* __restrict__ amb,
                                                          const double* __restrict__ grid, int32_t Q, int32_t n_qblk, int64_t n_units,
                                                          double* __restrict__ ll, int32_t* __restrict__ n_snp, int32_t* __restrict__ n_read) {
  __shared__ double s_log[DMX_LOG_TABLE_DOUBLES];
  __shared__ double s_pra[256][2];               // by read byte (allele << 7 | bq): {pR, pA}
  __shared__ AmbPair s_hdr[kAmbWaves][64];
  for (int i = threadIdx.x; i < DMX_LOG_TABLE_DOUBLES; i += 64 * kAmbWaves) s_log[i] = tabs[kLut + i];
  for (int i = threadIdx.x; i < 256; i += 64 * kAmbWaves) {
    const double mat = tabs[i & 127], e3 = tabs[128 + (i & 127)];
    s_pra[i][0] = (i >> 7) ? e3 : mat;
    s_pra[i][1] = (i >> 7) ? mat : e3;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t unit = (int64_t)blockIdx.x * kAmbWaves + wave;
  if (unit >= n_units) return;
  const int32_t cell = (int32_t)(unit / n_qblk), qb = (int32_t)(unit % n_qblk);
  const int32_t q = qb * 64 + lane;
  const int32_t v = assign[cell];
  double acc = 0.0;
  int32_t ns = 0, nr = 0;
  if (v >= 0) {
    AmbPair* hdr = s_hdr[wave];
    const double rho = q < Q ? grid[q] : 0.0;    // lanes past Q run along and write nothing
    const double om = 1.0 - rho, half = 0.5 * om;
    const DmxLogPins lk = dmx_log_pins();
    const int64_t p_beg = pv.cell_pair_off[cell], p_end = pv.cell_pair_off[cell + 1];
    int64_t rd_base = pv.cell_read_off[cell];
    for (int64_t p0 = p_beg; p0 < p_end; p0 += 64) {
      const int64_t p = p0 + lane;
      const bool in = p < p_end;
      const uint32_t n = in ? load_nrd(pv.pair_nrd, p, nrd_width) : 0u;
      const uint32_t incl = seg_scan_incl<64>(n);
      AmbPair h{};
      h.off = rd_base + (int64_t)(incl - n);
      rd_base += (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      if (n > 0) {
        const int32_t snp = pv.pair_snp ? pv.pair_snp[p] : (int32_t)(p - p_beg);
        const float* gr = g + ((size_t)snp * V + v) * 3;
        const float g0 = gr[0], g1 = gr[1], g2 = gr[2];
        h.g0 = g0; h.g1 = g1; h.g2 = g2;
        h.a = amb[snp];
        h.rd4 = load_rd4(pv, h.off, n);
        h.n = (g0 != 0.f || g1 != 0.f || g2 != 0.f) ? n : 0u;
      }
      hdr[lane] = h;
      DMX_WAVE_LDS_ORDER();
      const int cnt = (int)min<int64_t>(64, p_end - p0);
      for (int j = 0; j < cnt; ++j) {
        const uint32_t nj = (uint32_t)__builtin_amdgcn_readfirstlane((int)hdr[j].n);
        if (nj == 0) continue;
        const double ra = rho * hdr[j].a;
        const double p_0 = ra, p_1 = half + ra, p_2 = om + ra;
        const double q_0 = 1.0 - p_0, q_1 = 1.0 - p_1, q_2 = 1.0 - p_2;
        const int64_t off = hdr[j].off;
        uint32_t w = hdr[j].rd4;
        double pR = s_pra[w & 0xFF][0], pA = s_pra[w & 0xFF][1];
        double f0 = pR * q_0 + pA * p_0, f1 = pR * q_1 + pA * p_1, f2 = pR * q_2 + pA * p_2;
        if (nj >= 8) {                               // a pair that may be rescaled: f_g of a zero gp entry is 0, so that the scale follows the
          if (hdr[j].g0 == 0.0) f0 = 0.0;            // entries that count and nothing ignored can grow past them (0 x inf)
          if (hdr[j].g1 == 0.0) f1 = 0.0;
          if (hdr[j].g2 == 0.0) f2 = 0.0;
        }
        int32_t E = 0;
        for (uint32_t r = 1; r < nj; ++r) {
          if ((r & 3) == 0) w = load_rd4(pv, off + r, nj - r);
          const uint32_t byte = (w >> (8 * (r & 3))) & 0xFF;
          pR = s_pra[byte][0]; pA = s_pra[byte][1];
          f0 *= pR * q_0 + pA * p_0; f1 *= pR * q_1 + pA * p_1; f2 *= pR * q_2 + pA * p_2;
          if ((r & 7) == 7) {
            const double mx = fmax(f0, fmax(f1, f2));
            if (mx < kAmbRescaleBelow && mx > 0.0) {
              int e;
              (void)frexp(mx, &e);
              f0 = ldexp(f0, -e); f1 = ldexp(f1, -e); f2 = ldexp(f2, -e);
              E += e;
            }
          }
        }
        const double L = hdr[j].g0 * f0 + hdr[j].g1 * f1 + hdr[j].g2 * f2;
        double lg = dmx_log_is_special(L) ? log(L) : dmx_log_fast_pinned(L, s_log, lk);
        if (E != 0) lg = __builtin_fma((double)E, DMX_LOG_LN2HI, __builtin_fma((double)E, DMX_LOG_LN2LO, lg));
        acc += lg;
        ns += 1; nr += (int32_t)nj;
      }
      DMX_WAVE_LDS_ORDER();
    }
  }
  if (q < Q) ll[(size_t)cell * Q + q] = acc;
  if (qb == 0 && lane == 0) { n_snp[cell] = ns; n_read[cell] = nr; }
}

// ---- donor shares of a read pool (dmx_engine_census_step / dmx_engine_census) -----------------------------------
// Every stored read of a group of barcodes is a draw from a mixture of the V donors with shares w.  One pass at w gives, per group,
//   acc[v] = sum over pairs of (1 - d[i][v]) sR + d[i][v] sA,  sR = sum over the pair's reads of pR / P_r,  sA = sum of pA / P_r,
//   LL = sum of log P_r,  P_r = pR (1 - A_i) + pA A_i,  A_i = sum over v, ascending, of w[v] d[i][v]
// (every product and sum rounded on its own: the build has no contraction).  The summation plan depends on the pileup, the group's own
// members and V only: a group's barcodes in ascending cell id are cut into chunks of kCenChunk; one wavefront walks a chunk's barcodes in
// that order and each barcode's pairs in stored order, 64 pairs (a tile) at a time.
//   Phase 1, lane = pair: read count and read offset by a DPP scan, the serial V-long dot product A_i with w in LDS, then the pair's
//   reads: two divisions and one dmx_log per read; a lane keeps a running LL and its counts; sR, sA and the SNP go to the tile in LDS.
//   Phase 2, lane = donor (blocks of 64 up to V): the lane adds the tile's pairs in order to its donor's sum, which lives in LDS
//   between tiles.  A pair without stored reads or at an invalid SNP has sR = sA = 0 and adds +0.  For V <= 32 the 64 lanes form
//   nsub = 64 / Vq sets of Vq lanes (Vq the power of two >= V); set s adds the tile's pairs s, s + nsub, ... and the sets' sums are
//   added in set order at the end of the chunk.
// At the end of the chunk the 64 lanes' LL are added serially in lane order.  k_census_fold adds a group's chunk partials: chunk c goes
// to accumulator c mod 8 in chunk order, then ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)).  No floating-point atomics anywhere.
constexpr int kCenWaves = 4;                     // wavefronts (chunks) per workgroup; they share the log and read tables
constexpr int kCenChunk = 4;                     // barcodes per chunk
constexpr int kCenMaxV = 1024, kCenMaxG = 1024;
struct CenChunk { int32_t g, beg, cnt, pad; };   // group, first index into the group-sorted cell list, barcodes
struct CenPair { double sR, sA; int32_t snp, pad; };

// d[i][v] = (gp1 / 2 + gp2) / (gp0 + gp1 + gp2) in float64; a row whose sum is not a positive finite number gets d = 0 and clears the
// SNP's valid flag (every lane that clears it stores the same byte).
__global__ __launch_bounds__(256) void k_census_dosage(const float* __restrict__ g, int64_t n, int32_t V, double* __restrict__ d,
                                                       uint8_t* __restrict__ valid) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const double g0 = g[3 * t], g1 = g[3 * t + 1], g2 = g[3 * t + 2];
  const double den = (g0 + g1) + g2;
  const bool ok = den > 0.0 && den < INFINITY;
  d[t] = ok ? (g1 * 0.5 + g2) / den : 0.0;
  if (!ok) valid[t / V] = 0;
}

__global__ __launch_bounds__(64 * kCenWaves) void k_census_step(PileupView pv, int nrd_width, const double* __restrict__ tabs,
                                                              const double* __restrict__ d, const uint8_t* __restrict__ valid, int32_t V,
                                                              const int32_t* __restrict__ order, const CenChunk* __restrict__ chunks,
                                                              int32_t n_chunks, const uint8_t* __restrict__ active,
                                                              const double* __restrict__ w, double* __restrict__ part,
                                                              int64_t* __restrict__ pcnt) {
  extern __shared__ double s_dyn[];              // per wavefront: w[Vp] | acc[Vp], Vp = V rounded up to 64
  __shared__ double s_log[DMX_LOG_TABLE_DOUBLES];
  __shared__ double s_pra[256][2];               // by read byte (allele << 7 | bq): {pR, pA}
  __shared__ CenPair s_tile[kCenWaves][64];
  __shared__ int64_t s_cnt[kCenWaves][64][2];
  for (int i = threadIdx.x; i < DMX_LOG_TABLE_DOUBLES; i += 64 * kCenWaves) s_log[i] = tabs[kLut + i];
  for (int i = threadIdx.x; i < 256; i += 64 * kCenWaves) {
    const double mat = tabs[i & 127], e3 = tabs[128 + (i & 127)];
    s_pra[i][0] = (i >> 7) ? e3 : mat;
    s_pra[i][1] = (i >> 7) ? mat : e3;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int32_t chunk = (int32_t)blockIdx.x * kCenWaves + wave;
  if (chunk >= n_chunks) return;
  const int32_t grp = __builtin_amdgcn_readfirstlane(chunks[chunk].g);
  const int32_t c_beg = __builtin_amdgcn_readfirstlane(chunks[chunk].beg), c_cnt = __builtin_amdgcn_readfirstlane(chunks[chunk].cnt);
  if (!active[grp]) return;                      // a frozen group: its partials and results stay
  const int32_t Vp = (V + 63) & ~63;
  int qshift = 6;                                // V <= 32: Vq = the power of two >= V, nsub = 64 / Vq lane sets share phase 2
  while (qshift > 0 && (1 << (qshift - 1)) >= V) --qshift;
  const int32_t Vq = 1 << qshift, nsub = 64 >> qshift;
  double* sw = s_dyn + (size_t)wave * 2 * Vp;
  double* sa = sw + Vp;
  for (int32_t v = lane; v < Vp; v += 64) { sw[v] = v < V ? w[(size_t)grp * V + v] : 0.0; sa[v] = 0.0; }
  DMX_WAVE_LDS_ORDER();
  CenPair* tile = s_tile[wave];
  const DmxLogPins lk = dmx_log_pins();
  double ll = 0.0;
  int64_t nr = 0, np = 0;
  for (int32_t c = 0; c < c_cnt; ++c) {
    const int32_t cell = __builtin_amdgcn_readfirstlane(order[c_beg + c]);
    const int64_t p_beg = pv.cell_pair_off[cell], p_end = pv.cell_pair_off[cell + 1];
    int64_t rd_base = pv.cell_read_off[cell];
    for (int64_t p0 = p_beg; p0 < p_end; p0 += 64) {
      const int64_t p = p0 + lane;
      const bool in = p < p_end;
      const uint32_t n = in ? load_nrd(pv.pair_nrd, p, nrd_width) : 0u;
      const uint32_t incl = seg_scan_incl<64>(n);
      const int64_t off = rd_base + (int64_t)(incl - n);
      rd_base += (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      const int32_t snp = in ? (pv.pair_snp ? pv.pair_snp[p] : (int32_t)(p - p_beg)) : 0;
      const bool use = n > 0 && valid[snp];
      const double* dr = d + (size_t)snp * V;
      double A = 0.0;
      for (int32_t v = 0; v < V; ++v) A = A + sw[v] * dr[v];
      const double q = 1.0 - A;
      double sR = 0.0, sA = 0.0;
      if (use) {
        uint32_t wd = 0;
        for (uint32_t r = 0; r < n; ++r) {
          if ((r & 3) == 0) wd = load_rd4(pv, off + r, n - r);
          const uint32_t byte = (wd >> (8 * (r & 3))) & 0xFF;
          const double pR = s_pra[byte][0], pA = s_pra[byte][1];
          const double P = pR * q + pA * A;
          sR += pR / P; sA += pA / P;
          ll += dmx_log_is_special(P) ? log(P) : dmx_log_fast_pinned(P, s_log, lk);
        }
        nr += (int64_t)n; np += 1;
      }
      CenPair t;
      t.sR = sR; t.sA = sA; t.snp = use ? snp : 0; t.pad = 0;
      tile[lane] = t;
      DMX_WAVE_LDS_ORDER();
      const int cnt = (int)min<int64_t>(64, p_end - p0);
      if (nsub > 1) {                              // V <= 32: nsub sets of Vq lanes, set s takes the tile's pairs s, s + nsub, ...
        const int32_t v = lane & (Vq - 1), vv = v < V ? v : 0;
        double a = sa[lane];
#pragma unroll 4
        for (int j = lane >> qshift; j < cnt; j += nsub) {
          const double dv = d[(size_t)tile[j].snp * V + vv];
          a += (1.0 - dv) * tile[j].sR + dv * tile[j].sA;
        }
        sa[lane] = a;
      } else {
        for (int32_t v0 = 0; v0 < Vp; v0 += 64) {
          const int32_t v = v0 + lane, vv = v < V ? v : 0;   // lanes past V run along on donor 0; their sums are never written out
          double a = sa[v];
#pragma unroll 4
          for (int j = 0; j < cnt; ++j) {
            const double dv = d[(size_t)tile[j].snp * V + vv];
            a += (1.0 - dv) * tile[j].sR + dv * tile[j].sA;
          }
          sa[v] = a;
        }
      }
      DMX_WAVE_LDS_ORDER();
    }
  }
  double* out = part + (size_t)chunk * ((size_t)V + 1);
  if (nsub > 1) {
    if (lane < V) {
      double a = 0.0;
      for (int s = 0; s < nsub; ++s) a += sa[s * Vq + lane];
      out[lane] = a;
    }
  } else {
    for (int32_t v = lane; v < V; v += 64) out[v] = sa[v];
  }
  tile[lane].sR = ll;
  s_cnt[wave][lane][0] = nr; s_cnt[wave][lane][1] = np;
  DMX_WAVE_LDS_ORDER();
  if (lane == 0) {
    double s = 0.0;
    int64_t a = 0, b = 0;
    for (int j = 0; j < 64; ++j) { s += tile[j].sR; a += s_cnt[wave][j][0]; b += s_cnt[wave][j][1]; }
    out[V] = s;
    pcnt[2 * (size_t)chunk] = a; pcnt[2 * (size_t)chunk + 1] = b;
  }
}

// One workgroup per group: out[g] = acc[V] | LL | gap | N (as a double), cnt[g] = {reads, pairs}.  gap = N (max_v acc_v / N - 1), 0 for
// a group without a counted read.
__global__ __launch_bounds__(256) void k_census_fold(const double* __restrict__ part, const int64_t* __restrict__ pcnt,
                                                     const int32_t* __restrict__ chunk_off, const uint8_t* __restrict__ active, int32_t V,
                                                     double* __restrict__ out, int64_t* __restrict__ cnt) {
  __shared__ double s_max[256];
  const int32_t g = blockIdx.x, tid = threadIdx.x;
  if (!active[g]) return;
  const int32_t c0 = chunk_off[g], c1 = chunk_off[g + 1];
  const size_t stride = (size_t)V + 1;
  auto fold8 = [&](int32_t col) {
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int32_t c = c0; c < c1; c += 8) {
#pragma unroll
      for (int k = 0; k < 8; ++k) if (c + k < c1) a[k] += part[(size_t)(c + k) * stride + col];
    }
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  };
  double* o = out + (size_t)g * ((size_t)V + 3);
  double mx = 0.0;
  for (int32_t v = tid; v < V; v += 256) {
    const double x = fold8(v);
    o[v] = x;
    mx = fmax(mx, x);
  }
  s_max[tid] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) s_max[tid] = fmax(s_max[tid], s_max[tid + s]);
    __syncthreads();
  }
  if (tid == 0) {
    int64_t nr = 0, np = 0;
    for (int32_t c = c0; c < c1; ++c) { nr += pcnt[2 * (size_t)c]; np += pcnt[2 * (size_t)c + 1]; }
    const double N = (double)nr;
    o[V] = fold8(V);
    o[V + 1] = nr > 0 ? N * (s_max[0] / N - 1.0) : 0.0;
    o[V + 2] = N;
    cnt[2 * (size_t)g] = nr; cnt[2 * (size_t)g + 1] = np;
  }
}

// ---- census uncertainty: observed information and per-barcode scores (dmx_engine_census_fisher) ------------------
// At shares w, a stored read r of pair (b, i) has the step's quotients tR = pR / P_r and tA = pA / P_r.  Per pair sRR = sum tR tR,
// sRA = sum tR tA, sAA = sum tA tA (reads in stored order), and with e_v = 1 - d[i][v]
//   H[g][v][u]  = sum over the pairs of group g of ((e_v e_u) sRR + (e_v d_u + d_v e_u) sRA) + (d_v d_u) sAA,  v <= u,
//   score[b][v] = sum over the pairs of barcode b of e_v sR + d_v sA                     (the step's acc, kept per barcode),
// every product and sum rounded on its own.  The E = V (V + 1) / 2 upper-triangle entries are numbered row-major and cut into blocks of
// kFisBlock = 2048: one wavefront per (chunk, entry block), the chunks being census_prepare's.  A lane owns the entries
// block * 2048 + k * 64 + lane, k < 32, and keeps their 32 running sums in registers over the whole chunk.
//   Phase 1, lane = pair: k_census_step's phase 1 (same statements, hence the same A_i, P_r, tR, tA; no log), plus the three sums of
//   products.  Every entry block of a chunk repeats it: phase 2b is V (V + 1) / 2 terms per pair, phase 1 a handful per read.
//   Phase 2a, entry block 0 only, lane = donor: k_census_step's phase 2 with the sums reset at a barcode's first tile and stored at its
//   last (for V <= 32 the lane sets' sums are added in set order there).  Lane 0 adds the 64 positions' counted reads of the barcode.
//   Phase 2b, lane = entry: for each k the lane adds the tile's pairs in stored order to its entry's sum; the d rows come from global
//   memory (L1 / L2: a tile touches at most 64 rows), the pair's five sums are broadcast from LDS.
// A barcode's pairs go 64 at a time, barcodes in chunk order, so an entry's chunk partial is one serial sum.  k_census_fisher_fold adds a
// group's chunk partials in k_census_fold's eight-accumulator order and writes both triangles.  No floating-point atomics.
constexpr int kFisBlock = 2048, kFisPerLane = kFisBlock / 64;
constexpr int kFisMaxV = 128;
struct FisPair { double sR, sA, sRR, sRA, sAA; int32_t snp, pad; };

// Entry e of the row-major upper triangle of a V x V matrix -> (v, u), v <= u.  Row r starts at r V - r (r - 1) / 2.
__device__ __forceinline__ void fis_decode(int32_t e, int32_t V, int32_t& v, int32_t& u) {
  const float t = (float)(2 * V + 1);
  int32_t r = (int32_t)((t - sqrtf(fmaxf(t * t - 8.0f * (float)e, 0.0f))) * 0.5f);
  r = max(0, min(r, V - 1));
  while (r > 0 && r * V - r * (r - 1) / 2 > e) --r;
  while (r < V - 1 && (r + 1) * V - (r + 1) * r / 2 <= e) ++r;
  v = r; u = r + (e - (r * V - r * (r - 1) / 2));
}

__global__ __launch_bounds__(64 * kCenWaves) void k_census_fisher(PileupView pv, int nrd_width, const double* __restrict__ tabs,
                                                                const double* __restrict__ d, const uint8_t* __restrict__ valid, int32_t V,
                                                                const int32_t* __restrict__ order, const CenChunk* __restrict__ chunks,
                                                                int32_t n_chunks, int32_t n_blocks, const double* __restrict__ w,
                                                                double* __restrict__ hpart, double* __restrict__ score,
                                                                int64_t* __restrict__ n_read_b) {
  __shared__ double s_pra[256][2];               // by read byte (allele << 7 | bq): {pR, pA}
  __shared__ FisPair s_tile[kCenWaves][64];
  __shared__ double s_w[kCenWaves][kFisMaxV], s_a[kCenWaves][kFisMaxV];
  __shared__ int64_t s_nr[kCenWaves][64];
  for (int i = threadIdx.x; i < 256; i += 64 * kCenWaves) {
    const double mat = tabs[i & 127], e3 = tabs[128 + (i & 127)];
    s_pra[i][0] = (i >> 7) ? e3 : mat;
    s_pra[i][1] = (i >> 7) ? mat : e3;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int32_t unit = (int32_t)blockIdx.x * kCenWaves + wave;          // (the host checks that n_chunks x n_blocks fits)
  if (unit >= n_chunks * n_blocks) return;
  const int32_t chunk = __builtin_amdgcn_readfirstlane(unit / n_blocks), eb = unit - chunk * n_blocks;
  const int32_t grp = __builtin_amdgcn_readfirstlane(chunks[chunk].g);
  const int32_t c_beg = __builtin_amdgcn_readfirstlane(chunks[chunk].beg), c_cnt = __builtin_amdgcn_readfirstlane(chunks[chunk].cnt);
  const int32_t E = V * (V + 1) / 2, e0 = eb * kFisBlock;
  const int32_t Vp = (V + 63) & ~63;
  int qshift = 6;                                // V <= 32: Vq = the power of two >= V, nsub = 64 / Vq lane sets share phase 2a
  while (qshift > 0 && (1 << (qshift - 1)) >= V) --qshift;
  const int32_t Vq = 1 << qshift, nsub = 64 >> qshift;
  double* sw = s_w[wave];
  double* sa = s_a[wave];
  for (int32_t v = lane; v < Vp; v += 64) sw[v] = v < V ? w[(size_t)grp * V + v] : 0.0;
  DMX_WAVE_LDS_ORDER();
  const int kmax = min(kFisPerLane, (E - e0 + 63) / 64);   // the k that hold an entry of this block
  uint32_t pv8[kFisPerLane / 4], pu8[kFisPerLane / 4];     // v and u (< 128: a byte each) of this lane's entries; a lane past E runs along on entry 0
  double hh[kFisPerLane];
#pragma unroll
  for (int k4 = 0; k4 < kFisPerLane / 4; ++k4) {
    uint32_t a = 0u, b = 0u;
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
      const int32_t e = e0 + (k4 * 4 + t) * 64 + lane;
      int32_t v = 0, u = 0;
      if (k4 * 4 + t < kmax) fis_decode(e < E ? e : 0, V, v, u);
      a |= (uint32_t)v << (8 * t);
      b |= (uint32_t)u << (8 * t);
    }
    pv8[k4] = a; pu8[k4] = b;
  }
#pragma unroll
  for (int k = 0; k < kFisPerLane; ++k) hh[k] = 0.0;
  FisPair* tile = s_tile[wave];
  for (int32_t c = 0; c < c_cnt; ++c) {
    const int32_t cell = __builtin_amdgcn_readfirstlane(order[c_beg + c]);
    const int64_t p_beg = pv.cell_pair_off[cell], p_end = pv.cell_pair_off[cell + 1];
    int64_t rd_base = pv.cell_read_off[cell];
    int64_t nr = 0;
    if (eb == 0) {
      for (int32_t v = lane; v < Vp; v += 64) sa[v] = 0.0;
      DMX_WAVE_LDS_ORDER();
    }
    for (int64_t p0 = p_beg; p0 < p_end; p0 += 64) {
      const int64_t p = p0 + lane;
      const bool in = p < p_end;
      const uint32_t n = in ? load_nrd(pv.pair_nrd, p, nrd_width) : 0u;
      const uint32_t incl = seg_scan_incl<64>(n);
      const int64_t off = rd_base + (int64_t)(incl - n);
      rd_base += (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      const int32_t snp = in ? (pv.pair_snp ? pv.pair_snp[p] : (int32_t)(p - p_beg)) : 0;
      const bool use = n > 0 && valid[snp];
      const double* dr = d + (size_t)snp * V;
      double A = 0.0;
      for (int32_t v = 0; v < V; ++v) A = A + sw[v] * dr[v];
      const double q = 1.0 - A;
      double sR = 0.0, sA = 0.0, sRR = 0.0, sRA = 0.0, sAA = 0.0;
      if (use) {
        uint32_t wd = 0;
        for (uint32_t r = 0; r < n; ++r) {
          if ((r & 3) == 0) wd = load_rd4(pv, off + r, n - r);
          const uint32_t byte = (wd >> (8 * (r & 3))) & 0xFF;
          const double pR = s_pra[byte][0], pA = s_pra[byte][1];
          const double P = pR * q + pA * A;
          const double tR = pR / P, tA = pA / P;
          sR += tR; sA += tA;
          sRR += tR * tR; sRA += tR * tA; sAA += tA * tA;
        }
        nr += (int64_t)n;
      }
      FisPair t;
      t.sR = sR; t.sA = sA; t.sRR = sRR; t.sRA = sRA; t.sAA = sAA; t.snp = use ? snp : 0; t.pad = 0;
      tile[lane] = t;
      DMX_WAVE_LDS_ORDER();
      const int cnt = (int)min<int64_t>(64, p_end - p0);
      if (eb == 0) {                               // phase 2a: the barcode's score row
        if (nsub > 1) {
          const int32_t v = lane & (Vq - 1), vv = v < V ? v : 0;
          double a = sa[lane];
#pragma unroll 4
          for (int j = lane >> qshift; j < cnt; j += nsub) {
            const double dv = d[(size_t)tile[j].snp * V + vv];
            a += (1.0 - dv) * tile[j].sR + dv * tile[j].sA;
          }
          sa[lane] = a;
        } else {
          for (int32_t v0 = 0; v0 < Vp; v0 += 64) {
            const int32_t v = v0 + lane, vv = v < V ? v : 0;
            double a = sa[v];
#pragma unroll 4
            for (int j = 0; j < cnt; ++j) {
              const double dv = d[(size_t)tile[j].snp * V + vv];
              a += (1.0 - dv) * tile[j].sR + dv * tile[j].sA;
            }
            sa[v] = a;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < kFisPerLane; ++k) {      // phase 2b: lane = entry
        if (k < kmax) {
          uint32_t wv = pv8[k >> 2], wu = pu8[k >> 2];
          asm volatile("" : "+v"(wv), "+v"(wu));   // (unpacked here, per tile: 64 hoisted offsets would cost the registers the sums need)
          const uint32_t v = (wv >> (8 * (k & 3))) & 0xFFu, u = (wu >> (8 * (k & 3))) & 0xFFu;
          double h = hh[k];
#pragma unroll 2
          for (int j = 0; j < cnt; ++j) {
            const double* row = d + (size_t)tile[j].snp * V;
            const double dv = row[v], du = row[u];
            const double ev = 1.0 - dv, eu = 1.0 - du;
            h += ((ev * eu) * tile[j].sRR + (ev * du + dv * eu) * tile[j].sRA) + (dv * du) * tile[j].sAA;
          }
          hh[k] = h;
        }
      }
      DMX_WAVE_LDS_ORDER();
    }
    if (eb == 0) {                                 // the barcode's last tile is done: its score row and counted reads
      double* out = score + (size_t)cell * V;
      if (nsub > 1) {
        if (lane < V) {
          double a = 0.0;
          for (int s = 0; s < nsub; ++s) a += sa[s * Vq + lane];
          out[lane] = a;
        }
      } else {
        for (int32_t v = lane; v < V; v += 64) out[v] = sa[v];
      }
      s_nr[wave][lane] = nr;
      DMX_WAVE_LDS_ORDER();
      if (lane == 0) {
        int64_t a = 0;
        for (int j = 0; j < 64; ++j) a += s_nr[wave][j];
        n_read_b[cell] = a;
      }
      DMX_WAVE_LDS_ORDER();
    }
  }
  double* out = hpart + (size_t)chunk * (size_t)E;
#pragma unroll
  for (int k = 0; k < kFisPerLane; ++k) {
    const int32_t e = e0 + k * 64 + lane;
    if (e < E) out[e] = hh[k];
  }
}

// One workgroup per (group, 256 entries): H[g][v][u] = H[g][u][v] = the chunk partials of entry (v, u) folded as k_census_fold does.
__global__ __launch_bounds__(256) void k_census_fisher_fold(const double* __restrict__ hpart, const int32_t* __restrict__ chunk_off, int32_t V,
                                                            double* __restrict__ H) {
  const int32_t g = blockIdx.x, E = V * (V + 1) / 2;
  const int32_t e = (int32_t)blockIdx.y * 256 + (int32_t)threadIdx.x;
  if (e >= E) return;
  const int32_t c0 = chunk_off[g], c1 = chunk_off[g + 1];
  double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int32_t c = c0; c < c1; c += 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) if (c + k < c1) a[k] += hpart[(size_t)(c + k) * (size_t)E + e];
  }
  const double x = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  int32_t v, u;
  fis_decode(e, V, v, u);
  double* Hg = H + (size_t)g * V * V;
  Hg[(size_t)v * V + u] = x;
  Hg[(size_t)u * V + v] = x;
}

// ---- ambient-aware doublet profile (dmx_engine_ambient_doublet) --------------------------------------------------
// For a barcode b, a candidate pair (v1, v2), a mixing share alpha of v2 and a grid point rho:
//   p_lm = (1 - rho) (0.5 l + (m - l) 0.5 alpha) + rho a_i,   f_lm = product over the pair's stored reads of pR (1 - p_lm) + pA p_lm,
//   LL = sum over b's pairs, in stored (ascending SNP) order, of log(sum_l sum_m gp[i][v1][l] gp[i][v2][m] f_lm)  (l-major, m-minor).
// k_ambient's skeleton: one wavefront per (barcode, alpha, block of 64 grid points), one lane per grid point, PT pair headers staged in LDS
// per trip.  The nine f_lm depend on the pair, alpha and rho but not on the candidate: a lane forms them once per pair and folds them
// into one running sum per candidate (nine exact float32 x float32 weights, nine multiply-adds, one log), so a further candidate costs
// the fold and not the read loop.  The candidates' two gp rows (2 x 3 float32) ride in the staged header; a header's mask has bit c set
// when both rows of candidate c have a non-zero entry, and a pair with mask 0 or no stored read is skipped.  The nine mixing
// constants are wave-uniform and sit in scalar registers.
// Range: a pair of fewer than 8 reads cannot leave the normal range (one read scales f by >= 2^-44) and takes the plain path.  A deeper
// pair keeps one exponent PER ENTRY: every 8 reads an f_lm below 2^-300 is scaled by the exact power of two that brings it to
// [0.5, 1) and the exponent goes to E_lm; a candidate takes E = max E_lm over its entries with a non-zero weight, sums
// w_lm f_lm 2^(E_lm - E) (exact shifts; an entry more than ~700 binades below the largest adds nothing) and gets log(L) + E ln 2.  A
// shared exponent would not do here: for an ALT-heavy pair the hom-REF x hom-REF entry is thousands of binades below the largest of the
// nine, and it is the only one a hom-REF x hom-REF candidate counts.
// Nothing crosses lanes and every entry is one serial sum: its bits depend on b's data, (v1, v2), alpha and rho only (the CC / PT
// instantiation changes which slots exist and how many headers a trip stages, not an entry's operations or their order).
constexpr int kAmbDblWaves = 4;
constexpr int kAmbDblMaxCand = 8, kAmbDblMaxAlpha = 8;
template <int CC> struct AmbDblPair { double a; int64_t off; uint32_t n, rd4, mask, pad; float gp[CC][6]; };   // n = 0: skipped

__device__ __forceinline__ double amb_uniform(double x) {          // a wave-uniform double into a scalar register pair
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}

// One pair: the nine read products of this lane's rho, then the fold into the running sums of the candidates in `mask`.
template <int CC, bool DEEP>
__device__ __forceinline__ void amb_dbl_pair(const PileupView& pv, const AmbDblPair<CC>& h, uint32_t nj, uint32_t mask, const double (&cm)[9],
                                             double rho, double om, const double (*s_pra)[2], const double* s_log, const DmxLogPins& lk,
                                             double (&acc)[CC]) {
  const double ra = rho * h.a;
  double pp[9], qq[9], f[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) { pp[k] = om * cm[k] + ra; qq[k] = 1.0 - pp[k]; }
  const int64_t off = h.off;
  uint32_t w = h.rd4;
  double pR = s_pra[w & 0xFF][0], pA = s_pra[w & 0xFF][1];
#pragma unroll
  for (int k = 0; k < 9; ++k) f[k] = pR * qq[k] + pA * pp[k];
  int32_t E[9];
  if (DEEP) {
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = 0;
  }
  for (uint32_t r = 1; r < nj; ++r) {
    if ((r & 3) == 0) w = load_rd4(pv, off + r, nj - r);
    const uint32_t byte = (w >> (8 * (r & 3))) & 0xFF;
    pR = s_pra[byte][0]; pA = s_pra[byte][1];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] *= pR * qq[k] + pA * pp[k];
    if (DEEP && (r & 7) == 7) {
#pragma unroll
      for (int k = 0; k < 9; ++k)
        if (f[k] < kAmbRescaleBelow && f[k] > 0.0) {
          int e;
          (void)frexp(f[k], &e);
          f[k] = ldexp(f[k], -e);
          E[k] += e;
        }
    }
  }
#pragma unroll
  for (int c = 0; c < CC; ++c) {
    if (!((mask >> c) & 1u)) continue;
    double g1[3], g2[3];
#pragma unroll
    for (int l = 0; l < 3; ++l) { g1[l] = (double)h.gp[c][l]; g2[l] = (double)h.gp[c][3 + l]; }
    double L = 0.0;
    int32_t em = 0;
    if (DEEP) {
      em = INT32_MIN / 2;
#pragma unroll
      for (int k = 0; k < 9; ++k)
        if (g1[k / 3] * g2[k % 3] != 0.0 && f[k] > 0.0) em = max(em, E[k]);
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double wk = g1[k / 3] * g2[k % 3];                 // float32 x float32: exact in float64
        const double t = wk != 0.0 ? wk * ldexp(f[k], max(E[k] - em, -1100)) : 0.0;
        L = k == 0 ? t : L + t;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double t = (g1[k / 3] * g2[k % 3]) * f[k];
        L = k == 0 ? t : L + t;
      }
    }
    double lg = dmx_log_is_special(L) ? log(L) : dmx_log_fast_pinned(L, s_log, lk);
    if (DEEP && em != 0) lg = __builtin_fma((double)em, DMX_LOG_LN2HI, __builtin_fma((double)em, DMX_LOG_LN2LO, lg));
    acc[c] += lg;
  }
}

template <int CC, int PT>
__global__ __launch_bounds__(64 * kAmbDblWaves) void k_ambient_dbl(PileupView pv, int nrd_width, const double* __restrict__ tabs, const float* __restrict__ g,
                                                                 int32_t V, const int32_t* __restrict__ cand, int32_t C, const double* __restrict__ amb,
                                                                 const double* __restrict__ alpha, int32_t A, const double* __restrict__ grid, int32_t Q,
                                                                 int32_t n_qblk, int64_t n_units, double* __restrict__ ll, int32_t* __restrict__ n_snp,
                                                                 int32_t* __restrict__ n_read) {
  static_assert(CC >= 1 && CC <= kAmbDblMaxCand && PT >= 1 && PT <= 64, "candidate slots / staged headers per trip");
  __shared__ double s_log[DMX_LOG_TABLE_DOUBLES];
  __shared__ double s_pra[256][2];               // by read byte (allele << 7 | bq): {pR, pA}
  __shared__ AmbDblPair<CC> s_hdr[kAmbDblWaves][PT];
  for (int i = threadIdx.x; i < DMX_LOG_TABLE_DOUBLES; i += 64 * kAmbDblWaves) s_log[i] = tabs[kLut + i];
  for (int i = threadIdx.x; i < 256; i += 64 * kAmbDblWaves) {
    const double mat = tabs[i & 127], e3 = tabs[128 + (i & 127)];
    s_pra[i][0] = (i >> 7) ? e3 : mat;
    s_pra[i][1] = (i >> 7) ? mat : e3;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t unit = (int64_t)blockIdx.x * kAmbDblWaves + wave;
  if (unit >= n_units) return;
  const int32_t qb = (int32_t)(unit % n_qblk), ai = (int32_t)((unit / n_qblk) % A), cell = (int32_t)(unit / ((int64_t)n_qblk * A));
  const int32_t q = qb * 64 + lane;
  int32_t v1[CC], v2[CC], ns[CC], nr[CC];
  double acc[CC];
  uint32_t used = 0;
#pragma unroll
  for (int c = 0; c < CC; ++c) {
    v1[c] = -1; v2[c] = -1; ns[c] = 0; nr[c] = 0; acc[c] = 0.0;
    if (c < C) {
      v1[c] = cand[((size_t)cell * C + c) * 2];
      v2[c] = cand[((size_t)cell * C + c) * 2 + 1];
      if (v1[c] >= 0) used |= 1u << c;
    }
  }
  if (used) {
    AmbDblPair<CC>* hdr = s_hdr[wave];
    const double rho = q < Q ? grid[q] : 0.0;    // lanes past Q run along and write nothing
    const double om = 1.0 - rho;
    const double al = alpha[ai];
    double cm[9];
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
      for (int m = 0; m < 3; ++m) cm[l * 3 + m] = amb_uniform(0.5 * l + (m - l) * 0.5 * al);
    const DmxLogPins lk = dmx_log_pins();
    const int64_t p_beg = pv.cell_pair_off[cell], p_end = pv.cell_pair_off[cell + 1];
    int64_t rd_base = pv.cell_read_off[cell];
    for (int64_t p0 = p_beg; p0 < p_end; p0 += PT) {
      const int64_t p = p0 + lane;
      const bool in = lane < PT && p < p_end;
      const uint32_t n = in ? load_nrd(pv.pair_nrd, p, nrd_width) : 0u;
      const uint32_t incl = seg_scan_incl<64>(n);
      const int64_t off = rd_base + (int64_t)(incl - n);
      rd_base += (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      if (lane < PT) {
        AmbDblPair<CC>& h = hdr[lane];
        uint32_t mask = 0;
        if (n > 0) {
          const int32_t snp = pv.pair_snp ? pv.pair_snp[p] : (int32_t)(p - p_beg);
          const float* gs = g + (size_t)snp * V * 3;
#pragma unroll
          for (int c = 0; c < CC; ++c) {
            if (!((used >> c) & 1u)) continue;
            const float* r1 = gs + (size_t)v1[c] * 3;
            const float* r2 = gs + (size_t)v2[c] * 3;
            const float x0 = r1[0], x1 = r1[1], x2 = r1[2], y0 = r2[0], y1 = r2[1], y2 = r2[2];
            h.gp[c][0] = x0; h.gp[c][1] = x1; h.gp[c][2] = x2; h.gp[c][3] = y0; h.gp[c][4] = y1; h.gp[c][5] = y2;
            if ((x0 != 0.f || x1 != 0.f || x2 != 0.f) && (y0 != 0.f || y1 != 0.f || y2 != 0.f)) mask |= 1u << c;
          }
          h.a = amb[snp];
          h.rd4 = load_rd4(pv, off, n);
        }
        h.off = off;
        h.mask = mask;
        h.n = mask ? n : 0u;
      }
      DMX_WAVE_LDS_ORDER();
      const int cnt = (int)min<int64_t>(PT, p_end - p0);
      for (int j = 0; j < cnt; ++j) {
        const uint32_t nj = (uint32_t)__builtin_amdgcn_readfirstlane((int)hdr[j].n);
        if (nj == 0) continue;
        const uint32_t mask = (uint32_t)__builtin_amdgcn_readfirstlane((int)hdr[j].mask);
        if (nj < 8) amb_dbl_pair<CC, false>(pv, hdr[j], nj, mask, cm, rho, om, s_pra, s_log, lk, acc);
        else amb_dbl_pair<CC, true>(pv, hdr[j], nj, mask, cm, rho, om, s_pra, s_log, lk, acc);
#pragma unroll
        for (int c = 0; c < CC; ++c)
          if ((mask >> c) & 1u) { ns[c] += 1; nr[c] += (int32_t)nj; }
      }
      DMX_WAVE_LDS_ORDER();
    }
  }
#pragma unroll
  for (int c = 0; c < CC; ++c) {
    if (c >= C) continue;
    const size_t o = (size_t)cell * C + c;
    if (q < Q) ll[(o * A + ai) * Q + q] = acc[c];
    if (ai == 0 && qb == 0 && lane == 0) { n_snp[o] = ns[c]; n_read[o] = nr[c]; }
  }
}

// ---- goodness of fit (dmx_engine_fit) -----------------------------------------------------------------------------
// For a barcode b with the hypothesis (v1, v2, alpha, rho): over b's pairs, the log-likelihood c0 = log L(x) of the first m = min(n, M)
// stored reads' allele pattern x, and the mean and variance that log L(y) has when y is drawn from Pr(y) = L(y) / sum L(y') over the 2^m
// patterns (include/dmx.h states the operations).  k_ambient's skeleton — the log table and the phred tables in LDS, 64 pair headers per
// trip, read offsets by the DPP scan — but lane = pair: one wavefront per used barcode, lane l takes pairs l, l + 64, ... of the barcode
// in ascending order and keeps its own serial sums; at the end the 64 lanes' sums are added serially in lane order by lane 0 (no
// floating-point atomics, nothing from another barcode).  A lane holds mat / err3 of its m reads and p_c / q_c / W_c of the NC = 3
// (singlet) or 9 (doublet) components in registers, and, where NC * MM <= 36, t_r(c, 0 / 1) as well (KEEP); the doublet kernels for
// M > 4 form t_r from mat, err3, p_c and q_c per factor (three FP64 operations, not one; same operations, same bits).  Every array is
// indexed by unrolled constants only, the pattern's bits select by v_cndmask: no scratch.  The pattern loop runs to 2^mmax, mmax the
// tile's largest m (wave-uniform); lanes of smaller m sit out the rest (DESIGN.md section 26 says what that costs).
constexpr int kFitWaves = 4;                     // wavefronts (barcodes) per workgroup; they share the log and phred tables
constexpr int kFitMaxReads = 8;

template <int NC, int MM, bool KEEP>
__device__ __forceinline__ double fit_pattern(uint32_t y, uint32_t m, int mmax, const double (&t0)[KEEP ? MM * NC : 1],
                                              const double (&t1)[KEEP ? MM * NC : 1], const double (&mat)[MM], const double (&e3)[MM],
                                              const double (&pp)[NC], const double (&qq)[NC], const double (&W)[NC]) {
  double L = 0.0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    double F = 1.0;
#pragma unroll
    for (int r = 0; r < MM; ++r) {
      if (r < mmax) {                              // wave-uniform
        const bool alt = (y >> r) & 1u;
        double t;
        if constexpr (KEEP) {
          t = alt ? t1[r * NC + c] : t0[r * NC + c];   // (two arrays: one array indexed by 2 i + alt would be addressed, and live in scratch)
        } else {
          const double pR = alt ? e3[r] : mat[r], pA = alt ? mat[r] : e3[r];
          t = pR * qq[c] + pA * pp[c];
        }
        F = r == 0 ? t : ((uint32_t)r < m ? F * t : F);
      }
    }
    const double t = W[c] * F;
    L = c == 0 ? t : L + t;
  }
  return L;
}

template <bool DBL, int MM>
__global__ __launch_bounds__(64 * kFitWaves) void k_fit(PileupView pv, int nrd_width, const double* __restrict__ tabs, const float* __restrict__ g,
                                                      int32_t V, const int32_t* __restrict__ idx, int32_t n_idx, const int32_t* __restrict__ hyp,
                                                      const double* __restrict__ alpha, const double* __restrict__ rho,
                                                      const double* __restrict__ amb, int32_t M, int32_t B, double* __restrict__ out,
                                                      int32_t* __restrict__ cnt) {
  static_assert(MM == 1 || MM == 2 || MM == 4 || MM == 8, "reads per pair the instantiation holds");
  constexpr int NC = DBL ? 9 : 3;
  constexpr bool KEEP = NC * MM <= 36;
  __shared__ double s_log[DMX_LOG_TABLE_DOUBLES];
  __shared__ double s_me[128][2];                // by base quality: {mat, err / 3}
  __shared__ double s_red[kFitWaves][64][3];
  __shared__ int32_t s_cnt[kFitWaves][64][4];
  for (int i = threadIdx.x; i < DMX_LOG_TABLE_DOUBLES; i += 64 * kFitWaves) s_log[i] = tabs[kLut + i];
  for (int i = threadIdx.x; i < 128; i += 64 * kFitWaves) { s_me[i][0] = tabs[i]; s_me[i][1] = tabs[128 + i]; }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int32_t unit = (int32_t)blockIdx.x * kFitWaves + wave;
  if (unit >= n_idx) return;
  const int32_t cell = __builtin_amdgcn_readfirstlane(idx[unit]);
  const int32_t v1 = __builtin_amdgcn_readfirstlane(hyp[2 * (size_t)cell]);
  const int32_t v2 = DBL ? __builtin_amdgcn_readfirstlane(hyp[2 * (size_t)cell + 1]) : -1;
  const double rh = rho[cell], om = 1.0 - rh;
  double cm[NC];
  if (DBL) {
    const double al = alpha[cell];
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
      for (int k = 0; k < 3; ++k) cm[l * 3 + k] = 0.5 * l + (k - l) * 0.5 * al;
  } else {
#pragma unroll
    for (int c = 0; c < NC; ++c) cm[c] = 0.5 * c;
  }
  const DmxLogPins lk = dmx_log_pins();
  double obs = 0.0, mean = 0.0, var = 0.0;
  int32_t ns = 0, nr = 0, nt = 0, nz = 0;
  const int64_t p_beg = pv.cell_pair_off[cell], p_end = pv.cell_pair_off[cell + 1];
  int64_t rd_base = pv.cell_read_off[cell];
  for (int64_t p0 = p_beg; p0 < p_end; p0 += 64) {
    const int64_t p = p0 + lane;
    const bool in = p < p_end;
    const uint32_t n = in ? load_nrd(pv.pair_nrd, p, nrd_width) : 0u;
    const uint32_t incl = seg_scan_incl<64>(n);
    const int64_t off = rd_base + (int64_t)(incl - n);
    rd_base += (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    uint32_t m = 0, x = 0;                         // (the per-pair body from cm[] to the moments is k_site_partial's too: DESIGN.md says why it stays written twice)
    double W[NC], pp[NC], qq[NC], mat[MM], e3[MM];
#pragma unroll
    for (int c = 0; c < NC; ++c) { W[c] = 0.0; pp[c] = 0.0; qq[c] = 0.0; }
#pragma unroll
    for (int r = 0; r < MM; ++r) { mat[r] = 0.0; e3[r] = 0.0; }
    if (n > 0) {
      const int32_t snp = pv.pair_snp ? pv.pair_snp[p] : (int32_t)(p - p_beg);
      const float* gs = g + (size_t)snp * V * 3;
      const float* r1 = gs + (size_t)v1 * 3;
      const float x0 = r1[0], x1 = r1[1], x2 = r1[2];
      bool ok = x0 != 0.f || x1 != 0.f || x2 != 0.f;
      if (DBL) {
        const float* r2 = gs + (size_t)v2 * 3;
        const float y0 = r2[0], y1 = r2[1], y2 = r2[2];
        ok = ok && (y0 != 0.f || y1 != 0.f || y2 != 0.f);
        const double g1[3] = {(double)x0, (double)x1, (double)x2}, g2[3] = {(double)y0, (double)y1, (double)y2};
#pragma unroll
        for (int c = 0; c < NC; ++c) W[c] = g1[c / 3] * g2[c % 3];    // float32 x float32: exact in float64
      } else {
        W[0] = x0; W[1] = x1; W[2] = x2;
      }
      if (ok) {
        m = min(n, (uint32_t)M);
        const double ra = rh * amb[snp];
#pragma unroll
        for (int c = 0; c < NC; ++c) { pp[c] = om * cm[c] + ra; qq[c] = 1.0 - pp[c]; }
        const uint32_t w0 = load_rd4(pv, off, m);
        const uint32_t w1 = (MM > 4 && m > 4) ? load_rd4(pv, off + 4, m - 4) : 0u;
#pragma unroll
        for (int r = 0; r < MM; ++r) {
          const uint32_t byte = ((r < 4 ? w0 : w1) >> (8 * (r & 3))) & 0xFF;
          mat[r] = s_me[byte & 127][0]; e3[r] = s_me[byte & 127][1];
          if ((uint32_t)r < m) x |= (byte >> 7) << r;
        }
      }
    }
    int mmax = 0;
#pragma unroll
    for (int r = 0; r < MM; ++r)
      if (__ballot(m > (uint32_t)r)) mmax = r + 1;
    if (mmax == 0) continue;
    double t0[KEEP ? MM * NC : 1], t1[KEEP ? MM * NC : 1];
    if constexpr (KEEP) {
#pragma unroll
      for (int r = 0; r < MM; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          t0[r * NC + c] = mat[r] * qq[c] + e3[r] * pp[c];
          t1[r * NC + c] = e3[r] * qq[c] + mat[r] * pp[c];
        }
    } else {
      t0[0] = 0.0; t1[0] = 0.0;
    }
    bool live = m > 0;
    double c0 = 0.0;
    if (live) {
      const double Lx = fit_pattern<NC, MM, KEEP>(x, m, mmax, t0, t1, mat, e3, pp, qq, W);
      if (Lx == 0.0) { live = false; nz += 1; }
      else c0 = dmx_log_is_special(Lx) ? log(Lx) : dmx_log_fast_pinned(Lx, s_log, lk);
    }
    double S0 = 0.0, S1 = 0.0, S2 = 0.0;
    const uint32_t npat = live ? 1u << m : 0u, nmax = 1u << mmax;
    for (uint32_t y = 0; y < nmax; ++y) {
      if (y < npat) {
        const double L = fit_pattern<NC, MM, KEEP>(y, m, mmax, t0, t1, mat, e3, pp, qq, W);
        if (L != 0.0) {
          const double lg = dmx_log_is_special(L) ? log(L) : dmx_log_fast_pinned(L, s_log, lk);
          const double u = lg - c0;
          S0 += L; S1 += L * u; S2 += L * (u * u);
        }
      }
    }
    if (live) {
      if (S0 == 0.0 || !(fabs(S0) < INFINITY)) {
        nz += 1;
      } else {
        const double e1 = S1 / S0, d = S2 / S0 - e1 * e1;
        obs += c0; mean += c0 + e1; var += d > 0.0 ? d : 0.0;
        ns += 1; nr += (int32_t)m; nt += n > (uint32_t)M;
      }
    }
  }
  s_red[wave][lane][0] = obs; s_red[wave][lane][1] = mean; s_red[wave][lane][2] = var;
  s_cnt[wave][lane][0] = ns; s_cnt[wave][lane][1] = nr; s_cnt[wave][lane][2] = nt; s_cnt[wave][lane][3] = nz;
  DMX_WAVE_LDS_ORDER();
  if (lane == 0) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    int32_t k0 = 0, k1 = 0, k2 = 0, k3 = 0;
    for (int l = 0; l < 64; ++l) {
      a0 += s_red[wave][l][0]; a1 += s_red[wave][l][1]; a2 += s_red[wave][l][2];
      k0 += s_cnt[wave][l][0]; k1 += s_cnt[wave][l][1]; k2 += s_cnt[wave][l][2]; k3 += s_cnt[wave][l][3];
    }
    out[cell] = a0; out[(size_t)B + cell] = a1; out[2 * (size_t)B + cell] = a2;
    cnt[cell] = k0; cnt[(size_t)B + cell] = k1; cnt[2 * (size_t)B + cell] = k2; cnt[3 * (size_t)B + cell] = k3;
  }
}

// ---- site audit (dmx_engine_site_fit) ----------------------------------------------------------------------------
// k_fit's per-pair terms, summed per SNP instead of per barcode, with the pair's ALT excess k(x) - E k(y) and its variance beside them.
// Sum order (the contract): the used barcodes as dmx_engine_fit lists them (singlets, then doublets, ascending cell id each), each list
// cut into chunks of kSiteChunk; inside a chunk the terms are added in list order (k_site_partial), then the chunk partials in ascending
// chunk order (k_site_fold).  No floating-point atomics.  The slab table is the refinement's (k_snp_blocks at kRefSlabShift).
constexpr int kSiteChunk = 64;                   // used barcodes per chunk
struct SitePartial { double v[5]; int32_t n[5]; int32_t pad; };   // obs, mean, var, exc, vexc | n_cell, n_read, n_alt, n_trunc, n_zero
static_assert(sizeof(SitePartial) == 64, "partial rows of 64 bytes");

// One wavefront per (chunk, SNP slab), the chunk's barcodes one after another as k_refine_partial walks them; per barcode lane = pair
// over its pairs inside the slab, the per-pair body k_fit's (same operations, same bits: a pair's terms do not depend on which pairs
// share its tile).  Each lane adds its terms into the slab's LDS accumulators at its SNP: a barcode has at most one pair per SNP, so
// lanes never collide, and the LDS executes one wavefront's instructions in program order, so barcode b + 1 adds after barcode b.
// `members` / `chunk_beg` are the whole plan's; this launch covers chunks c0 + blockIdx.y and writes partial rows row0 + blockIdx.y.
template <bool DBL, int MM>
__global__ __launch_bounds__(64) void k_site_partial(PileupView pv, int nrd_width, const double* __restrict__ tabs, const float* __restrict__ g, int32_t V,
                                                     const int64_t* __restrict__ blk, int32_t nblk, const int32_t* __restrict__ members,
                                                     const int32_t* __restrict__ chunk_beg, int32_t c0, int32_t row0, const int32_t* __restrict__ hyp,
                                                     const double* __restrict__ alpha, const double* __restrict__ rho,
                                                     const double* __restrict__ amb, int32_t M, SitePartial* __restrict__ partial) {
  static_assert(MM == 1 || MM == 2 || MM == 4 || MM == 8, "reads per pair the instantiation holds");
  constexpr int NC = DBL ? 9 : 3;
  constexpr bool KEEP = NC * MM <= 36;
  __shared__ double s_log[DMX_LOG_TABLE_DOUBLES];
  __shared__ double s_me[128][2];                // by base quality: {mat, err / 3}
  __shared__ double s_v[5][kRefSlab];
  __shared__ int32_t s_n[5][kRefSlab];
  const int lane = threadIdx.x;
  const int32_t slab = blockIdx.x, chunk = c0 + (int32_t)blockIdx.y;
  const int32_t s0 = slab << kRefSlabShift;
  for (int i = lane; i < DMX_LOG_TABLE_DOUBLES; i += 64) s_log[i] = tabs[kLut + i];
  for (int i = lane; i < 128; i += 64) { s_me[i][0] = tabs[i]; s_me[i][1] = tabs[128 + i]; }
  for (int i = lane; i < kRefSlab; i += 64) {
#pragma unroll
    for (int j = 0; j < 5; ++j) { s_v[j][i] = 0.0; s_n[j][i] = 0; }
  }
  __syncthreads();
  const DmxLogPins lk = dmx_log_pins();
  const int32_t m_end = __builtin_amdgcn_readfirstlane(chunk_beg[chunk + 1]);
  for (int32_t mb = __builtin_amdgcn_readfirstlane(chunk_beg[chunk]); mb < m_end; ++mb) {
    const int32_t cell = __builtin_amdgcn_readfirstlane(members[mb]);
    const int32_t v1 = __builtin_amdgcn_readfirstlane(hyp[2 * (size_t)cell]);
    const int32_t v2 = DBL ? __builtin_amdgcn_readfirstlane(hyp[2 * (size_t)cell + 1]) : -1;
    const double rh = rho[cell], om = 1.0 - rh;
    double cm[NC];
    if (DBL) {
      const double al = alpha[cell];
#pragma unroll
      for (int l = 0; l < 3; ++l)
#pragma unroll
        for (int k = 0; k < 3; ++k) cm[l * 3 + k] = 0.5 * l + (k - l) * 0.5 * al;
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c) cm[c] = 0.5 * c;
    }
    const int64_t* bt = blk + ((size_t)cell * (nblk + 1) + slab) * 2;
    const int64_t p_end = bt[2], cell_p0 = pv.cell_pair_off[cell];
    int64_t rd_base = bt[1];
    for (int64_t p0 = bt[0]; p0 < p_end; p0 += 64) {
      const int64_t p = p0 + lane;
      const bool in = p < p_end;
      const uint32_t n = in ? load_nrd(pv.pair_nrd, p, nrd_width) : 0u;
      const int32_t snp = in ? (pv.pair_snp ? pv.pair_snp[p] : (int32_t)(p - cell_p0)) : 0;
      const uint32_t incl = seg_scan_incl<64>(n);
      const int64_t off = rd_base + (int64_t)(incl - n);
      rd_base += (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      const int k = snp - s0;                          // inside the slab by construction (pairs in ascending SNP order); checked all the same
      uint32_t m = 0, x = 0;                       // (the per-pair body from cm[] to the moments is k_fit's: DESIGN.md says why it stays written twice)
      double W[NC], pp[NC], qq[NC], mat[MM], e3[MM];
#pragma unroll
      for (int c = 0; c < NC; ++c) { W[c] = 0.0; pp[c] = 0.0; qq[c] = 0.0; }
#pragma unroll
      for (int r = 0; r < MM; ++r) { mat[r] = 0.0; e3[r] = 0.0; }
      if (n > 0 && (unsigned)k < (unsigned)kRefSlab) {
        const float* gs = g + (size_t)snp * V * 3;
        const float* r1 = gs + (size_t)v1 * 3;
        const float x0 = r1[0], x1 = r1[1], x2 = r1[2];
        bool ok = x0 != 0.f || x1 != 0.f || x2 != 0.f;
        if (DBL) {
          const float* r2 = gs + (size_t)v2 * 3;
          const float y0 = r2[0], y1 = r2[1], y2 = r2[2];
          ok = ok && (y0 != 0.f || y1 != 0.f || y2 != 0.f);
          const double g1[3] = {(double)x0, (double)x1, (double)x2}, g2[3] = {(double)y0, (double)y1, (double)y2};
#pragma unroll
          for (int c = 0; c < NC; ++c) W[c] = g1[c / 3] * g2[c % 3];    // float32 x float32: exact in float64
        } else {
          W[0] = x0; W[1] = x1; W[2] = x2;
        }
        if (ok) {
          m = min(n, (uint32_t)M);
          const double ra = rh * amb[snp];
#pragma unroll
          for (int c = 0; c < NC; ++c) { pp[c] = om * cm[c] + ra; qq[c] = 1.0 - pp[c]; }
          const uint32_t w0 = load_rd4(pv, off, m);
          const uint32_t w1 = (MM > 4 && m > 4) ? load_rd4(pv, off + 4, m - 4) : 0u;
#pragma unroll
          for (int r = 0; r < MM; ++r) {
            const uint32_t byte = ((r < 4 ? w0 : w1) >> (8 * (r & 3))) & 0xFF;
            mat[r] = s_me[byte & 127][0]; e3[r] = s_me[byte & 127][1];
            if ((uint32_t)r < m) x |= (byte >> 7) << r;
          }
        }
      }
      int mmax = 0;
#pragma unroll
      for (int r = 0; r < MM; ++r)
        if (__ballot(m > (uint32_t)r)) mmax = r + 1;
      if (mmax == 0) continue;
      double t0[KEEP ? MM * NC : 1], t1[KEEP ? MM * NC : 1];
      if constexpr (KEEP) {
#pragma unroll
        for (int r = 0; r < MM; ++r)
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            t0[r * NC + c] = mat[r] * qq[c] + e3[r] * pp[c];
            t1[r * NC + c] = e3[r] * qq[c] + mat[r] * pp[c];
          }
      } else {
        t0[0] = 0.0; t1[0] = 0.0;
      }
      bool live = m > 0, zero = false;
      double lc0 = 0.0;
      if (live) {
        const double Lx = fit_pattern<NC, MM, KEEP>(x, m, mmax, t0, t1, mat, e3, pp, qq, W);
        if (Lx == 0.0) { live = false; zero = true; }
        else lc0 = dmx_log_is_special(Lx) ? log(Lx) : dmx_log_fast_pinned(Lx, s_log, lk);
      }
      double S0 = 0.0, S1 = 0.0, S2 = 0.0, A1 = 0.0, A2 = 0.0;
      const uint32_t npat = live ? 1u << m : 0u, nmax = 1u << mmax;
      for (uint32_t y = 0; y < nmax; ++y) {
        if (y < npat) {
          const double L = fit_pattern<NC, MM, KEEP>(y, m, mmax, t0, t1, mat, e3, pp, qq, W);
          if (L != 0.0) {
            const double lg = dmx_log_is_special(L) ? log(L) : dmx_log_fast_pinned(L, s_log, lk);
            const double u = lg - lc0, ky = (double)__popc(y);
            S0 += L; S1 += L * u; S2 += L * (u * u);
            A1 += L * ky; A2 += L * (ky * ky);
          }
        }
      }
      if (live) {
        if (S0 == 0.0 || !(fabs(S0) < INFINITY)) {
          zero = true;
        } else {
          const double e1 = S1 / S0, d = S2 / S0 - e1 * e1;
          const double a1 = A1 / S0, da = A2 / S0 - a1 * a1;
          const int32_t kx = (int32_t)__popc(x);
          s_v[0][k] += lc0; s_v[1][k] += lc0 + e1; s_v[2][k] += d > 0.0 ? d : 0.0;
          s_v[3][k] += (double)kx - a1; s_v[4][k] += da > 0.0 ? da : 0.0;
          s_n[0][k] += 1; s_n[1][k] += (int32_t)m; s_n[2][k] += kx; s_n[3][k] += n > (uint32_t)M;
        }
      }
      if (zero) s_n[4][k] += 1;
      DMX_WAVE_LDS_ORDER();
    }
  }
  SitePartial* out = partial + (size_t)(row0 + (int32_t)blockIdx.y) * pv.S + s0;
  const int lim = min(kRefSlab, pv.S - s0);
  for (int i = lane; i < lim; i += 64) {
    SitePartial r;
#pragma unroll
    for (int j = 0; j < 5; ++j) { r.v[j] = s_v[j][i]; r.n[j] = s_n[j][i]; }
    r.pad = 0;
    out[i] = r;
  }
}

// One lane per SNP: adds the `nc` partial rows of this wave of chunks, in ascending chunk order, onto the running sums val[5][S] and
// cnt[5][S] (zeroed before the first wave).
__global__ __launch_bounds__(256) void k_site_fold(const SitePartial* __restrict__ partial, int32_t S, int32_t nc, double* __restrict__ val,
                                                   int32_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  double a[5];
  int32_t k[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) { a[j] = val[(size_t)j * S + i]; k[j] = cnt[(size_t)j * S + i]; }
  for (int32_t c = 0; c < nc; ++c) {
    const SitePartial& r = partial[(size_t)c * S + i];
#pragma unroll
    for (int j = 0; j < 5; ++j) { a[j] += r.v[j]; k[j] += r.n[j]; }
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) { val[(size_t)j * S + i] = a[j]; cnt[(size_t)j * S + i] = k[j]; }
}

// ---- continuous mixing share (dmx_engine_share_scan / dmx_engine_share_fit) ---------------------------------------
// Section 18's doublet likelihood LL(alpha) of a barcode and a pair (v1, v2) with its first and second derivative in alpha
// (include/dmx.h states the operations).  Per entry (l, m) the read loop keeps, beside the product f_lm and its exponent, S1 = sum u and
// S2 = sum u u of u = (pA - pR) / t over the reads; the three entries l = m have s_lm = 0 and take no quotient.  The power-of-two scale
// of a deep pair is common to L, L' and L'' and cancels in D1 = L' / L and D2 = L'' / L - D1 D1.
//   k_share_scan  alpha = 0, every partner of an anchor: p_lm does not depend on m there, so phase 1 (lane = pair) runs the read loop for
//                 the three l once per pair and leaves F_l, x = s S1 and y = x x - s s S2 of the six l != m entries in LDS; phase 2
//                 (lane = partner) folds the tile's pairs in stored order into the lane's own three sums: nine weights, two quotients, one
//                 log.  One wavefront per (barcode, anchor slot, block of 64 partners); nothing crosses lanes.
//   k_share_fit   one wavefront per (barcode, candidate), lane = pair as k_fit; the 64 lanes' sums are added serially in lane order by
//                 every lane (the same bits in each), and the safeguarded Newton iteration runs on the wave-uniform result.  The reads
//                 are read again each evaluation.
constexpr int kShareWaves = 4;
constexpr int kShareMaxAnchor = 4, kShareMaxCand = 8, kShareMaxSamples = 1024, kShareMaxIter = 200;
constexpr int kShareFitDoubles = 13, kShareFitInts = 4;   // per (b, c): alpha_hat | LL, LL', LL'' at alpha_hat, 0, 1, probe;  n_eval, status, n_snp, n_read
constexpr int32_t kShareNoExp = INT32_MIN / 2;

// The read loop of one pair over NE entries: f (with section 18's rescaling into E) and, for the entries with s != 0, S1 and S2.
template <int NE, bool DIAG>
__device__ __forceinline__ void share_reads(const PileupView& pv, int64_t off, uint32_t n, uint32_t w, const double (&pp)[NE], const double (&qq)[NE],
                                            const double (*s_pra)[2], double (&f)[NE], int32_t (&E)[NE], double (&S1)[NE], double (&S2)[NE]) {
#pragma unroll
  for (int k = 0; k < NE; ++k) { f[k] = 0.0; E[k] = 0; S1[k] = 0.0; S2[k] = 0.0; }
  for (uint32_t r = 0; r < n; ++r) {
    if (r > 0 && (r & 3) == 0) w = load_rd4(pv, off + r, n - r);
    const uint32_t byte = (w >> (8 * (r & 3))) & 0xFF;
    const double pR = s_pra[byte][0], pA = s_pra[byte][1];
    const double dlt = pA - pR;
#pragma unroll
    for (int k = 0; k < NE; ++k) {
      const double t = pR * qq[k] + pA * pp[k];
      f[k] = r == 0 ? t : f[k] * t;
      if (!DIAG || k % 4 != 0) {
        const double u = t != 0.0 ? dlt / t : 0.0;              // a factor 0 zeroes f: the entry adds nothing, whatever S1 and S2 hold
        S1[k] += u; S2[k] += u * u;
      }
    }
    if ((r & 7) == 7) {
#pragma unroll
      for (int k = 0; k < NE; ++k)
        if (f[k] < kAmbRescaleBelow && f[k] > 0.0) {
          int e;
          (void)frexp(f[k], &e);
          f[k] = ldexp(f[k], -e);
          E[k] += e;
        }
    }
  }
}

struct ShareScanPair { double F[3], x[6], y[6]; float g1[3]; int32_t snp, E; uint32_t n; };   // n = 0: skipped

__global__ __launch_bounds__(64 * kShareWaves) void k_share_scan(PileupView pv, int nrd_width, const double* __restrict__ tabs, const float* __restrict__ g,
                                                               int32_t V, const int32_t* __restrict__ anchors, int32_t T, const double* __restrict__ rho,
                                                               const double* __restrict__ amb, int32_t n_vblk, int64_t n_units,
                                                               double* __restrict__ out, int32_t* __restrict__ cnt) {
  __shared__ double s_log[DMX_LOG_TABLE_DOUBLES];
  __shared__ double s_pra[256][2];               // by read byte (allele << 7 | bq): {pR, pA}
  __shared__ ShareScanPair s_tile[kShareWaves][64];
  for (int i = threadIdx.x; i < DMX_LOG_TABLE_DOUBLES; i += 64 * kShareWaves) s_log[i] = tabs[kLut + i];
  for (int i = threadIdx.x; i < 256; i += 64 * kShareWaves) {
    const double mat = tabs[i & 127], e3 = tabs[128 + (i & 127)];
    s_pra[i][0] = (i >> 7) ? e3 : mat;
    s_pra[i][1] = (i >> 7) ? mat : e3;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t unit = (int64_t)blockIdx.x * kShareWaves + wave;
  if (unit >= n_units) return;
  const int32_t vb = (int32_t)(unit % n_vblk), slot = (int32_t)(unit / n_vblk);   // slot = b T + t
  const int32_t cell = slot / T;
  const int32_t v1 = __builtin_amdgcn_readfirstlane(anchors[slot]);
  if (v1 < 0) return;                              // (the call zeroed the outputs)
  const int32_t v = vb * 64 + lane;
  const bool active = v < V && v != v1;
  const int32_t vv = v < V ? v : 0;
  const double rh = amb_uniform(rho[cell]), om = 1.0 - rh;
  const double s1 = om * 0.5;                      // s_lm = s1 (m - l): exact multiples
  const DmxLogPins lk = dmx_log_pins();
  ShareScanPair* tile = s_tile[wave];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  int32_t ns = 0, nr = 0;
  const int64_t p_beg = pv.cell_pair_off[cell], p_end = pv.cell_pair_off[cell + 1];
  int64_t rd_base = pv.cell_read_off[cell];
  for (int64_t p0 = p_beg; p0 < p_end; p0 += 64) {
    const int64_t p = p0 + lane;
    const bool in = p < p_end;
    const uint32_t n = in ? load_nrd(pv.pair_nrd, p, nrd_width) : 0u;
    const uint32_t incl = seg_scan_incl<64>(n);
    const int64_t off = rd_base + (int64_t)(incl - n);
    rd_base += (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    {                                              // phase 1: lane = pair
      ShareScanPair h;
      h.n = 0; h.snp = 0; h.E = 0;
#pragma unroll
      for (int l = 0; l < 3; ++l) { h.F[l] = 0.0; h.g1[l] = 0.f; }
#pragma unroll
      for (int j = 0; j < 6; ++j) { h.x[j] = 0.0; h.y[j] = 0.0; }
      if (n > 0) {
        const int32_t snp = pv.pair_snp ? pv.pair_snp[p] : (int32_t)(p - p_beg);
        const float* r1 = g + ((size_t)snp * V + (size_t)v1) * 3;
        const float x0 = r1[0], x1 = r1[1], x2 = r1[2];
        if (x0 != 0.f || x1 != 0.f || x2 != 0.f) {
          const double ra = rh * amb[snp];
          double pp[3], qq[3], f[3], S1[3], S2[3];
          int32_t E[3];
#pragma unroll
          for (int l = 0; l < 3; ++l) { pp[l] = om * (0.5 * l) + ra; qq[l] = 1.0 - pp[l]; }
          share_reads<3, false>(pv, off, n, load_rd4(pv, off, n), pp, qq, s_pra, f, E, S1, S2);
          h.g1[0] = x0; h.g1[1] = x1; h.g1[2] = x2;
          int32_t em = kShareNoExp;
#pragma unroll
          for (int l = 0; l < 3; ++l)
            if (h.g1[l] != 0.f && f[l] > 0.0) em = max(em, E[l]);
#pragma unroll
          for (int l = 0; l < 3; ++l) h.F[l] = (h.g1[l] != 0.f && f[l] > 0.0) ? ldexp(f[l], max(E[l] - em, -1100)) : 0.0;
          int j = 0;
#pragma unroll
          for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int m = 0; m < 3; ++m) {
              if (m == l) continue;
              const double s = s1 * (double)(m - l);
              const double x = s * S1[l];
              h.x[j] = x; h.y[j] = x * x - (s * s) * S2[l];
              ++j;
            }
          h.snp = snp; h.E = em; h.n = n;
        }
      }
      ns += (int32_t)__builtin_popcountll(__ballot(h.n > 0));
      nr += (int32_t)(uint32_t)__builtin_amdgcn_readlane((int)seg_scan_incl<64>(h.n), 63);
      tile[lane] = h;
    }
    DMX_WAVE_LDS_ORDER();
    const int cnt_t = (int)min<int64_t>(64, p_end - p0);
    for (int j = 0; j < cnt_t; ++j) {                // phase 2: lane = partner
      const ShareScanPair& h = tile[j];
      const uint32_t nj = (uint32_t)__builtin_amdgcn_readfirstlane((int)h.n);
      if (nj == 0) continue;
      const float* r2 = g + ((size_t)h.snp * V + (size_t)vv) * 3;
      const float y0 = r2[0], y1 = r2[1], y2 = r2[2];
      if (!active || (y0 == 0.f && y1 == 0.f && y2 == 0.f)) continue;
      const double g1[3] = {(double)h.g1[0], (double)h.g1[1], (double)h.g1[2]}, g2[3] = {(double)y0, (double)y1, (double)y2};
      double L = 0.0, L1 = 0.0, L2 = 0.0;
      int o = 0;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double wk = g1[k / 3] * g2[k % 3];                   // float32 x float32: exact in float64
        const double t = wk != 0.0 ? wk * h.F[k / 3] : 0.0;
        L = k == 0 ? t : L + t;
        if (k % 4 != 0) {
          const double t1 = t * h.x[o], t2 = t * h.y[o];
          L1 = o == 0 ? t1 : L1 + t1;
          L2 = o == 0 ? t2 : L2 + t2;
          ++o;
        }
      }
      double lg = dmx_log_is_special(L) ? log(L) : dmx_log_fast_pinned(L, s_log, lk);
      const int32_t em = h.E;
      if (em != 0) lg = __builtin_fma((double)em, DMX_LOG_LN2HI, __builtin_fma((double)em, DMX_LOG_LN2LO, lg));
      const double d1 = L1 / L;
      a0 += lg; a1 += d1; a2 += L2 / L - d1 * d1;
    }
    DMX_WAVE_LDS_ORDER();
  }
  if (active) {
    double* o = out + ((size_t)slot * V + (size_t)v) * 3;
    o[0] = a0; o[1] = a1; o[2] = a2;
  }
  if (vb == 0 && lane == 0) { cnt[2 * (size_t)slot] = ns; cnt[2 * (size_t)slot + 1] = nr; }
}

// One evaluation of (LL, LL', LL'') at the share `al` for k_share_fit's wavefront; the results are wave-uniform.
__device__ __forceinline__ void share_fit_eval(const PileupView& pv, int nrd_width, const float* __restrict__ g, int32_t V, int32_t cell, int32_t v1,
                                            int32_t v2, double rh, const double* __restrict__ amb, double al, const double (*s_pra)[2],
                                            const double* s_log, double (*red)[3], int lane, double (&res)[3], int32_t& n_snp, int32_t& n_read) {
  const double om = 1.0 - rh, s1 = om * 0.5;
  double cm[9];
#pragma unroll
  for (int l = 0; l < 3; ++l)
#pragma unroll
    for (int m = 0; m < 3; ++m) cm[l * 3 + m] = amb_uniform(0.5 * l + ((m - l) * 0.5) * al);
  const DmxLogPins lk = dmx_log_pins();
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  int32_t ns = 0, nr = 0;
  const int64_t p_beg = pv.cell_pair_off[cell], p_end = pv.cell_pair_off[cell + 1];
  int64_t rd_base = pv.cell_read_off[cell];
  for (int64_t p0 = p_beg; p0 < p_end; p0 += 64) {
    const int64_t p = p0 + lane;
    const bool in = p < p_end;
    const uint32_t n = in ? load_nrd(pv.pair_nrd, p, nrd_width) : 0u;
    const uint32_t incl = seg_scan_incl<64>(n);
    const int64_t off = rd_base + (int64_t)(incl - n);
    rd_base += (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (n == 0) continue;
    const int32_t snp = pv.pair_snp ? pv.pair_snp[p] : (int32_t)(p - p_beg);
    const float* gs = g + (size_t)snp * V * 3;
    const float* r1 = gs + (size_t)v1 * 3;
    const float* r2 = gs + (size_t)v2 * 3;
    const float x0 = r1[0], x1 = r1[1], x2 = r1[2], y0 = r2[0], y1 = r2[1], y2 = r2[2];
    if (!((x0 != 0.f || x1 != 0.f || x2 != 0.f) && (y0 != 0.f || y1 != 0.f || y2 != 0.f))) continue;
    const double g1[3] = {(double)x0, (double)x1, (double)x2}, g2[3] = {(double)y0, (double)y1, (double)y2};
    const double ra = rh * amb[snp];
    double pp[9], qq[9], f[9], S1[9], S2[9];
    int32_t E[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { pp[k] = om * cm[k] + ra; qq[k] = 1.0 - pp[k]; }
    share_reads<9, true>(pv, off, n, load_rd4(pv, off, n), pp, qq, s_pra, f, E, S1, S2);
    int32_t em = kShareNoExp;
#pragma unroll
    for (int k = 0; k < 9; ++k)
      if (g1[k / 3] * g2[k % 3] != 0.0 && f[k] > 0.0) em = max(em, E[k]);
    double L = 0.0, L1 = 0.0, L2 = 0.0;
    int o = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const double wk = g1[k / 3] * g2[k % 3];                     // float32 x float32: exact in float64
      const double t = wk != 0.0 ? wk * ldexp(f[k], max(E[k] - em, -1100)) : 0.0;
      L = k == 0 ? t : L + t;
      if (k % 4 != 0) {
        const double s = s1 * (double)(k % 3 - k / 3);
        const double x = s * S1[k];
        const double y = x * x - (s * s) * S2[k];
        const double t1 = t * x, t2 = t * y;
        L1 = o == 0 ? t1 : L1 + t1;
        L2 = o == 0 ? t2 : L2 + t2;
        ++o;
      }
    }
    double lg = dmx_log_is_special(L) ? log(L) : dmx_log_fast_pinned(L, s_log, lk);
    if (em != 0) lg = __builtin_fma((double)em, DMX_LOG_LN2HI, __builtin_fma((double)em, DMX_LOG_LN2LO, lg));
    const double d1 = L1 / L;
    a0 += lg; a1 += d1; a2 += L2 / L - d1 * d1;
    ns += 1; nr += (int32_t)n;
  }
  DMX_WAVE_LDS_ORDER();                            // (the last evaluation's sums have been read by every lane)
  red[lane][0] = a0; red[lane][1] = a1; red[lane][2] = a2;
  DMX_WAVE_LDS_ORDER();
  double b0 = 0.0, b1 = 0.0, b2 = 0.0;
  for (int l = 0; l < 64; ++l) { b0 += red[l][0]; b1 += red[l][1]; b2 += red[l][2]; }
  res[0] = amb_uniform(b0); res[1] = amb_uniform(b1); res[2] = amb_uniform(b2);
  n_snp = (int32_t)__builtin_amdgcn_readlane((int)seg_scan_incl<64>((uint32_t)ns), 63);
  n_read = (int32_t)__builtin_amdgcn_readlane((int)seg_scan_incl<64>((uint32_t)nr), 63);
}

__device__ __forceinline__ bool share_finite3(const double (&r)[3]) { return fabs(r[0]) < INFINITY && fabs(r[1]) < INFINITY && fabs(r[2]) < INFINITY; }

__global__ __launch_bounds__(64 * kShareWaves) void k_share_fit(PileupView pv, int nrd_width, const double* __restrict__ tabs, const float* __restrict__ g,
                                                              int32_t V, const int32_t* __restrict__ cand, const double* __restrict__ rho,
                                                              const double* __restrict__ amb, double start, double tol, int32_t max_iter, double probe,
                                                              int64_t n_units, double* __restrict__ out, int32_t* __restrict__ outi) {
  __shared__ double s_log[DMX_LOG_TABLE_DOUBLES];
  __shared__ double s_pra[256][2];               // by read byte (allele << 7 | bq): {pR, pA}
  __shared__ double s_red[kShareWaves][64][3];
  for (int i = threadIdx.x; i < DMX_LOG_TABLE_DOUBLES; i += 64 * kShareWaves) s_log[i] = tabs[kLut + i];
  for (int i = threadIdx.x; i < 256; i += 64 * kShareWaves) {
    const double mat = tabs[i & 127], e3 = tabs[128 + (i & 127)];
    s_pra[i][0] = (i >> 7) ? e3 : mat;
    s_pra[i][1] = (i >> 7) ? mat : e3;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t unit = (int64_t)blockIdx.x * kShareWaves + wave;   // = b C + c
  if (unit >= n_units) return;
  const int32_t v1 = __builtin_amdgcn_readfirstlane(cand[2 * unit]), v2 = __builtin_amdgcn_readfirstlane(cand[2 * unit + 1]);
  if (v1 < 0) return;                              // (the call zeroed the outputs)
  const int32_t C = (int32_t)(n_units / pv.B), cell = (int32_t)(unit / C);
  const double rh = amb_uniform(rho[cell]);
  double r0[3] = {0.0, 0.0, 0.0}, r1[3] = {0.0, 0.0, 0.0}, rx[3] = {0.0, 0.0, 0.0}, rp[3] = {0.0, 0.0, 0.0}, res[3];
  double a = 0.0, ahat = 0.0, lo = 0.0, hi = 1.0;
  int32_t state = 0, n_eval = 0, it = 0, status = 0, n_snp = 0, n_read = 0, ks = 0, kr = 0;
  for (;;) {
    share_fit_eval(pv, nrd_width, g, V, cell, v1, v2, rh, amb, a, s_pra, s_log, s_red[wave], lane, res, ks, kr);
    bool done = false;
    if (state == 0) {                              // step 1: the two ends
      ++n_eval; n_snp = ks; n_read = kr;
      r0[0] = res[0]; r0[1] = res[1]; r0[2] = res[2];
      a = 1.0; state = 1;
    } else if (state == 1) {
      ++n_eval;
      r1[0] = res[0]; r1[1] = res[1]; r1[2] = res[2];
      const bool dn0 = r0[1] <= 0.0, up1 = r1[1] >= 0.0;
      int end = -1;
      if (!share_finite3(r0) || !share_finite3(r1)) end = 0;      // nothing to iterate on: reported at 0 with DMX_SHARE_NONFINITE
      else if (dn0 && up1) end = r1[0] > r0[0] ? 1 : 0;           // step 2 (a tie goes to 0)
      else if (dn0) end = 0;                                      // step 3
      else if (up1) end = 1;                                      // step 4
      if (end == 0) { ahat = 0.0; rx[0] = r0[0]; rx[1] = r0[1]; rx[2] = r0[2]; status = DMX_SHARE_AT_0; done = true; }
      else if (end == 1) { ahat = 1.0; rx[0] = r1[0]; rx[1] = r1[1]; rx[2] = r1[2]; status = DMX_SHARE_AT_1; done = true; }
      else { a = start; state = 2; }                              // step 5
    } else if (state == 2) {                       // steps 6 to 9
      ++n_eval; ++it;
      if (res[1] > 0.0) lo = a; else hi = a;
      double an = a - res[1] / res[2];
      if (!(res[2] < 0.0 && an > lo && an < hi)) an = (lo + hi) * 0.5;
      const bool conv = fabs(an - a) <= tol;
      if (conv || it >= max_iter) {
        if (!conv) status |= DMX_SHARE_NOT_CONVERGED;
        state = 3;
      }
      a = an;
    } else if (state == 3) {                       // step 10
      ++n_eval;
      ahat = a; rx[0] = res[0]; rx[1] = res[1]; rx[2] = res[2];
      status |= DMX_SHARE_INTERIOR;
      done = true;
    } else {                                       // the probe (not counted in n_eval)
      rp[0] = res[0]; rp[1] = res[1]; rp[2] = res[2];
      break;
    }
    if (done) {
      if (!(probe >= 0.0)) break;
      a = probe; state = 4;
    }
  }
  if (rx[2] >= 0.0) status |= DMX_SHARE_FLAT;
  if (!share_finite3(r0) || !share_finite3(r1) || !share_finite3(rx)) status |= DMX_SHARE_NONFINITE;
  if (lane == 0) {
    double* o = out + (size_t)unit * kShareFitDoubles;
    o[0] = ahat;
#pragma unroll
    for (int i = 0; i < 3; ++i) { o[1 + i] = rx[i]; o[4 + i] = r0[i]; o[7 + i] = r1[i]; o[10 + i] = rp[i]; }
    int32_t* oi = outi + (size_t)unit * kShareFitInts;
    oi[0] = n_eval; oi[1] = status; oi[2] = n_snp; oi[3] = n_read;
  }
}

// ---- triplet profile (dmx_engine_triplet) -------------------------------------------------------------------------
// For a barcode b, a base pair (v1, v2), a share triple (w1, w2, w3) and EVERY sample c of the pool as the third donor:
//   p_lmn = 0.5 (w1 l + w2 m + w3 n),   f_lmn = product over the pair's stored reads of pR (1 - p_lmn) + pA p_lmn,
//   u_n = sum_l sum_m gp[i][v1][l] gp[i][v2][m] f_lmn (l-major, m-minor),   L_c = sum_n gp[i][c][n] u_n,
//   LL[b][s][t][c] = sum over b's pairs, in stored (ascending SNP) order, of log(L_c).
// One wavefront per (barcode, slot, share triple, block of 64 NACC columns); kTripPT pair headers staged in LDS per trip, then three steps:
//   phase 1   lane (h, k), h = lane / 32, k = lane % 32 < 27: entry k = (l, m, n) of pair 2 i + h, i = 0 .. kTripPT / 2 - 1: the read loop with
//             the entry's own exponent, then the weighted entry gp[v1][l] gp[v2][m] f_lmn (float32 x float32: exact) and its exponent go to LDS;
//   fold      lane (j, n) < 3 kTripPT: u_n of pair j, nine terms in the contract's order, and its exponent, to LDS;
//   phase 2   one lane per third donor c: per pair three float32 of g[snp][c] (lanes 12 bytes apart), three multiply-adds on the
//             broadcast u_n, one log, into the lane's own accumulator (NACC of them: columns c0 + 64 a + lane).
// Range (section 18's scheme): a pair of fewer than 8 reads keeps every exponent 0.  A deeper pair scales an f_lmn below 2^-300 to
// [0.5, 1) every 8 reads and keeps the exponent per entry; u_n takes E_n = max over its entries with a non-zero weight and sums
// t 2^(E_lmn - E_n), L_c takes E = max E_n over the n with gp[c][n] != 0 and sums gp u_n 2^(E_n - E) (exact shifts; a term more than
// ~700 binades below the largest adds nothing), and the log gets E ln 2.  With every exponent 0 the shifts are by 0, so both depths
// run the same sums.  Nothing depends on what else is in the call: an entry's bits follow from b's data, (v1, v2), the share triple, c
// and V (which picks NACC and the column block) only.
constexpr int kTripWaves = 4, kTripPT = 16;
constexpr int kTripMaxSlot = 8, kTripMaxShare = 8, kTripMaxAcc = 4;
constexpr int32_t kTripNoExp = INT32_MIN / 2;                     // the exponent of an entry that is 0 or carries no weight
struct TripPair { int64_t off; uint32_t n, rd4; int32_t snp; float gp[6]; uint32_t pad; };   // n = 0: skipped; gp = rows v1, v2

template <int NACC>
__global__ __launch_bounds__(64 * kTripWaves) void k_triplet(PileupView pv, int nrd_width, const double* __restrict__ tabs, const float* __restrict__ g,
                                                           int32_t V, const int32_t* __restrict__ base, int32_t C, const double* __restrict__ shares,
                                                           int32_t T, int32_t n_vblk, int64_t n_units, double* __restrict__ ll,
                                                           int32_t* __restrict__ n_snp, int32_t* __restrict__ n_read) {
  static_assert(NACC >= 1 && NACC <= kTripMaxAcc && kTripPT % 2 == 0 && 3 * kTripPT <= 64, "accumulators per lane / staged headers per trip");
  __shared__ double s_log[DMX_LOG_TABLE_DOUBLES];
  __shared__ double s_pra[256][2];               // by read byte (allele << 7 | bq): {pR, pA}
  __shared__ TripPair s_hdr[kTripWaves][kTripPT];
  __shared__ double s_t[kTripWaves][kTripPT][27];    // weighted entries
  __shared__ int32_t s_te[kTripWaves][kTripPT][27];  // their exponents
  __shared__ double s_u[kTripWaves][kTripPT][3];
  __shared__ int32_t s_ue[kTripWaves][kTripPT][3];
  for (int i = threadIdx.x; i < DMX_LOG_TABLE_DOUBLES; i += 64 * kTripWaves) s_log[i] = tabs[kLut + i];
  for (int i = threadIdx.x; i < 256; i += 64 * kTripWaves) {
    const double mat = tabs[i & 127], e3 = tabs[128 + (i & 127)];
    s_pra[i][0] = (i >> 7) ? e3 : mat;
    s_pra[i][1] = (i >> 7) ? mat : e3;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t unit = (int64_t)blockIdx.x * kTripWaves + wave;
  if (unit >= n_units) return;
  const int32_t vb = (int32_t)(unit % n_vblk), ti = (int32_t)((unit / n_vblk) % T);
  const int64_t slot = unit / ((int64_t)n_vblk * T);               // cell * C + s
  const int32_t cell = (int32_t)(slot / C);
  const int32_t c0 = vb * (64 * NACC) + lane;
  const int32_t v1 = __builtin_amdgcn_readfirstlane(base[slot * 2]), v2 = __builtin_amdgcn_readfirstlane(base[slot * 2 + 1]);
  double acc[NACC];
  int32_t ns[NACC], nr[NACC];
#pragma unroll
  for (int a = 0; a < NACC; ++a) { acc[a] = 0.0; ns[a] = 0; nr[a] = 0; }
  if (v1 >= 0) {
    TripPair* hdr = s_hdr[wave];
    double (*st)[27] = s_t[wave];
    int32_t (*ste)[27] = s_te[wave];
    double (*su)[3] = s_u[wave];
    int32_t (*sue)[3] = s_ue[wave];
    // phase 1's entry of this lane
    const int h = lane >> 5, k = lane & 31;
    const bool ent = k < 27;
    const int el = ent ? k / 9 : 0, em = ent ? (k / 3) % 3 : 0, en = ent ? k % 3 : 0;
    const double w1 = shares[3 * ti], w2 = shares[3 * ti + 1], w3 = shares[3 * ti + 2];
    const double pk = 0.5 * (w1 * (double)el + w2 * (double)em + w3 * (double)en), qk = 1.0 - pk;
    // the fold's (pair, n) of this lane
    const int fj = lane / 3, fn = lane - 3 * fj;
    const DmxLogPins lk = dmx_log_pins();
    const int64_t p_beg = pv.cell_pair_off[cell], p_end = pv.cell_pair_off[cell + 1];
    int64_t rd_base = pv.cell_read_off[cell];
    for (int64_t p0 = p_beg; p0 < p_end; p0 += kTripPT) {
      const int64_t p = p0 + lane;
      const bool in = lane < kTripPT && p < p_end;
      const uint32_t n = in ? load_nrd(pv.pair_nrd, p, nrd_width) : 0u;
      const uint32_t incl = seg_scan_incl<64>(n);
      const int64_t off = rd_base + (int64_t)(incl - n);
      rd_base += (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      if (lane < kTripPT) {
        TripPair& hd = hdr[lane];
        bool both = false;
        int32_t snp = 0;
        if (n > 0) {
          snp = pv.pair_snp ? pv.pair_snp[p] : (int32_t)(p - p_beg);
          const float* gs = g + (size_t)snp * V * 3;
          const float* r1 = gs + (size_t)v1 * 3;
          const float* r2 = gs + (size_t)v2 * 3;
          const float x0 = r1[0], x1 = r1[1], x2 = r1[2], y0 = r2[0], y1 = r2[1], y2 = r2[2];
          hd.gp[0] = x0; hd.gp[1] = x1; hd.gp[2] = x2; hd.gp[3] = y0; hd.gp[4] = y1; hd.gp[5] = y2;
          both = (x0 != 0.f || x1 != 0.f || x2 != 0.f) && (y0 != 0.f || y1 != 0.f || y2 != 0.f);
          hd.rd4 = load_rd4(pv, off, n);
        }
        hd.off = off;
        hd.snp = snp;
        hd.n = both ? n : 0u;
      }
      DMX_WAVE_LDS_ORDER();
      const int cnt = (int)min<int64_t>(kTripPT, p_end - p0);
      // phase 1: two pairs side by side
      for (int jj = 0; jj < cnt; jj += 2) {
        const int j = jj + h;
        const uint32_t nj = (ent && j < cnt) ? hdr[j].n : 0u;
        if (nj > 0) {
          const int64_t roff = hdr[j].off;
          uint32_t w = hdr[j].rd4;
          double f = s_pra[w & 0xFF][0] * qk + s_pra[w & 0xFF][1] * pk;
          int32_t E = 0;
          const bool deep = nj >= 8;
          for (uint32_t r = 1; r < nj; ++r) {
            if ((r & 3) == 0) w = load_rd4(pv, roff + r, nj - r);
            const uint32_t byte = (w >> (8 * (r & 3))) & 0xFF;
            f *= s_pra[byte][0] * qk + s_pra[byte][1] * pk;
            if (deep && (r & 7) == 7 && f < kAmbRescaleBelow && f > 0.0) {
              int e;
              (void)frexp(f, &e);
              f = ldexp(f, -e);
              E += e;
            }
          }
          const double wk = (double)hdr[j].gp[el] * (double)hdr[j].gp[3 + em];   // float32 x float32: exact in float64
          const double t = wk * f;
          st[j][k] = t;
          ste[j][k] = t > 0.0 ? E : kTripNoExp;
        }
      }
      DMX_WAVE_LDS_ORDER();
      // fold: u_n of pair fj
      if (fj < cnt && hdr[fj].n > 0) {
        int32_t En = kTripNoExp;
#pragma unroll
        for (int x = 0; x < 9; ++x) En = max(En, ste[fj][3 * x + fn]);
        if (En == kTripNoExp) En = 0;
        double u = 0.0;
#pragma unroll
        for (int x = 0; x < 9; ++x) {
          const double t = ldexp(st[fj][3 * x + fn], max(ste[fj][3 * x + fn] - En, -1100));
          u = x == 0 ? t : u + t;
        }
        su[fj][fn] = u;
        sue[fj][fn] = u > 0.0 ? En : kTripNoExp;
      }
      DMX_WAVE_LDS_ORDER();
      // phase 2: every third donor of this unit's columns
      for (int j = 0; j < cnt; ++j) {
        const uint32_t nj = (uint32_t)__builtin_amdgcn_readfirstlane((int)hdr[j].n);
        if (nj == 0) continue;
        const int32_t snp = __builtin_amdgcn_readfirstlane(hdr[j].snp);
        const double u0 = amb_uniform(su[j][0]), u1 = amb_uniform(su[j][1]), u2 = amb_uniform(su[j][2]);
        const int32_t e0 = __builtin_amdgcn_readfirstlane(sue[j][0]), e1 = __builtin_amdgcn_readfirstlane(sue[j][1]),
                      e2 = __builtin_amdgcn_readfirstlane(sue[j][2]);
        const float* gs = g + (size_t)snp * V * 3;
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
          const int32_t c = c0 + 64 * a;
          const float* gr = gs + (size_t)(c < V ? c : 0) * 3;    // lanes past V run along and write nothing
          const float g0 = gr[0], g1 = gr[1], g2 = gr[2];
          const bool nz = g0 != 0.f || g1 != 0.f || g2 != 0.f;
          double L;
          int32_t E = 0;
          if (nj < 8) {
            L = (double)g0 * u0 + (double)g1 * u1 + (double)g2 * u2;
          } else {
            E = kTripNoExp;
            if (g0 != 0.f) E = max(E, e0);
            if (g1 != 0.f) E = max(E, e1);
            if (g2 != 0.f) E = max(E, e2);
            if (E == kTripNoExp) E = 0;
            // (a u_n that carries no weight may sit far ABOVE the scale: its term is 0, not 0 x inf)
            const double t0 = g0 != 0.f ? (double)g0 * ldexp(u0, max(e0 - E, -1100)) : 0.0;
            const double t1 = g1 != 0.f ? (double)g1 * ldexp(u1, max(e1 - E, -1100)) : 0.0;
            const double t2 = g2 != 0.f ? (double)g2 * ldexp(u2, max(e2 - E, -1100)) : 0.0;
            L = t0 + t1 + t2;
          }
          if (!nz) L = 1.0;
          double lg = dmx_log_is_special(L) ? log(L) : dmx_log_fast_pinned(L, s_log, lk);
          if (E != 0) lg = __builtin_fma((double)E, DMX_LOG_LN2HI, __builtin_fma((double)E, DMX_LOG_LN2LO, lg));
          if (nz) { acc[a] += lg; ns[a] += 1; nr[a] += (int32_t)nj; }
        }
      }
      DMX_WAVE_LDS_ORDER();
    }
  }
#pragma unroll
  for (int a = 0; a < NACC; ++a) {
    const int32_t c = c0 + 64 * a;
    if (c >= V) continue;
    ll[((size_t)slot * T + ti) * V + c] = acc[a];
    if (ti == 0) { n_snp[(size_t)slot * V + c] = ns[a]; n_read[(size_t)slot * V + c] = nr[a]; }
  }
}

// SNP-minor copies for dense pileups: gT[r][s] = g[s][r] (r = k*3+l, float32 as stored) and g0T[l][s] = gp0s[s][l].
__global__ void k_transpose_geno(const float* __restrict__ g, const double* __restrict__ gp0, int32_t S, int32_t V,
                                 float* __restrict__ gT, double* __restrict__ g0T) {
  const int nrow = V * 3;
  const int64_t n = (int64_t)S * nrow;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = i % S;
    const int r = (int)(i / S);
    gT[i] = g[(size_t)s * nrow + r];
    if (r < 3) g0T[i] = gp0[(size_t)s * 3 + r];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// K2, generic form (any V, any A).  One cell per workgroup.  Accumulator q of the cell (q < V*V*A: (j,k,n) row-major,
// then A entries for llks00) lives in lane q % 256, register q / 256; grids with more than NACC*256 accumulators are cut into
// slabs of that many, one workgroup (blockIdx.y) per slab, each repeating the cheap phase 1 for itself.
//   phase 1  lane (pair ti, alpha n): the 9 mixture likelihoods pG[n][l][m] of that pair, reads in UMI order, with the
//            one-max-across-all-alphas renormalisation after every read (:600-663); A is padded to a power of two so the
//            A lanes of a pair sit together in a wavefront and share their max by butterfly shuffles;
//   phase 2  every accumulator adds log(sum_lm ...) for the tile's pairs in ascending SNP order (:671-709).
template <typename NRD, int NACC, bool FIXUP>
__global__ __launch_bounds__(kThreads) void k_doublet_generic(PileupView pv, const float* __restrict__ g,
                                                              const double* __restrict__ gp0,
                                                              const double* __restrict__ lut,
                                                              const double* __restrict__ alpha,
                                                              const int32_t* __restrict__ sched, int32_t V, int32_t A,
                                                              int32_t A_pad, int32_t TP, double* __restrict__ grid,
                                                              double* __restrict__ l00,
                                                              uint8_t* __restrict__ flagged) {
  // FIXUP: second pass behind the fast kernels — only cells in which one of them met a log() argument outside the normal
  // positive range (flagged[cell] != 0) are recomputed, with ocml's log() for exact log(0) / log(nan) semantics.  The pass is
  // launched with a small fixed grid whose workgroups stride over the cells, and it ends at once when no cell of the launch was
  // flagged at all (flag_cell also raises the launch-wide word in front of the array): nothing to fix costs ~2 us instead of a
  // dispatch of B workgroups.  The first pass (FIXUP = false) is launched with one workgroup per cell: one trip through the loop.
  if (FIXUP && !flags_any(flagged)) return;
  __shared__ double s_lut[kTab2];
  __shared__ double s_pG[kThreads * 9];
  __shared__ int32_t s_snp[32];
  __shared__ uint32_t s_cnt[32];
  __shared__ int64_t s_off[32];

  const int t = threadIdx.x;
  stage_k2_tables(s_lut, lut, t, kThreads);
  const double* s_log = s_lut + kLut2;
  for (int32_t bx = (int32_t)blockIdx.x; bx < pv.B; bx += (int32_t)gridDim.x) {
  if (FIXUP && !flagged[sched[bx]]) continue;
  const int32_t cell = sched[bx];
  const int64_t p_beg = pv.cell_pair_off[cell];
  const int64_t np = pv.cell_pair_off[cell + 1] - p_beg;
  int64_t rd_base = pv.cell_read_off[cell];
  const NRD* __restrict__ nrd = (const NRD*)pv.pair_nrd;

  // phase-1 identity and the per-(l,m) mixing weights of this lane's alpha (:613)
  const int ti1 = t / A_pad, n1 = t % A_pad;
  const bool lane1 = (ti1 < TP) && (n1 < A);
  double wA[9], wR[9];
  {
    const double al = lane1 ? alpha[n1] : 0.0;
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const double p = 0.5 * l + (m - l) * 0.5 * al;
        wA[l * 3 + m] = p;
        wR[l * 3 + m] = 1.0 - p;
      }
  }

  // phase-2 identity
  const int32_t nAB = V * V * A;
  const int32_t nacc = nAB + A;
  const int32_t q0 = (int32_t)blockIdx.y * NACC * kThreads;      // first accumulator of this workgroup's slab
  bool ok = true;              // every log() argument so far was a normal positive double (the fast path's domain)
  uint32_t code[NACC];         // (j << 20) | (k << 8) | n ; j = 0xFFF marks an llks00 entry; ~0u = no accumulator
  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const int32_t q = q0 + t + i * kThreads;
    acc[i] = 0.0;
    if (q < nAB) {
      const int32_t n = q % A, jk = q / A;
      code[i] = ((uint32_t)(jk / V) << 20) | ((uint32_t)(jk % V) << 8) | (uint32_t)n;
    } else if (q < nacc) {
      code[i] = (0xFFFu << 20) | (uint32_t)(q - nAB);
    } else {
      code[i] = ~0u;
    }
  }
  __syncthreads();

  for (int64_t base = 0; base < np; base += TP) {
    const int tp = (int)min((int64_t)TP, np - base);
    // pair headers of the tile
    if (t < 32) {
      const bool v = t < tp;
      const uint32_t n = v ? (uint32_t)nrd[p_beg + base + t] : 0u;
      uint32_t incl = n;
#pragma unroll
      for (int d = 1; d < 32; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d, 32);
        if (t >= d) incl += y;
      }
      if (v) {
        s_cnt[t] = n;
        s_off[t] = rd_base + (int64_t)(incl - n);
        s_snp[t] = pv.pair_snp ? pv.pair_snp[p_beg + base + t] : (int32_t)(base + t);
      }
    }
    __syncthreads();
    rd_base = s_off[tp - 1] + (int64_t)s_cnt[tp - 1];     // first read byte of the next tile, for every lane

    // ---- phase 1
    {
      const bool on = lane1 && ti1 < tp;
      const uint32_t cnt = on ? s_cnt[ti1] : 0u;
      const int64_t off = on ? s_off[ti1] : 0;
      const uint32_t rd4 = load_rd4(pv, off, cnt);       // the first four read bytes in one load (one dependent latency instead of four)
      double pG[9];
      const double mx = pair_values_open<9, 0, true>(pv, cnt, off, rd4, s_lut, wA, wR, n1, pG, nullptr, on, A_pad);
      if (on) {
        const double y = rcp_refined(mx);                                   // numerators >= 1e-6, mx in [1e-6, 1+1e-6]
#pragma unroll
        for (int i = 0; i < 9; ++i) s_pG[(ti1 * A + n1) * 9 + i] = div_by(pG[i], mx, y);   // :656-663
      }
    }
    __syncthreads();

    // ---- phase 2
    for (int ti = 0; ti < tp; ++ti) {
      const int32_t snp = s_snp[ti];
      const float* __restrict__ grow = g + (size_t)snp * V * 3;
      const double* __restrict__ g0 = gp0 + (size_t)snp * 3;
#pragma unroll
      for (int i = 0; i < NACC; ++i) {
        const uint32_t cd = code[i];
        if (cd == ~0u) continue;
        const int32_t j = (cd >> 20) & 0xFFF, k = (cd >> 8) & 0xFFF, n = cd & 0xFF;
        double a[3], b[3];
        if (j == 0xFFF) {
          a[0] = b[0] = g0[0]; a[1] = b[1] = g0[1]; a[2] = b[2] = g0[2];   // gp00 = gp0s[l]*gp0s[m]  (:555)
        } else {
          a[0] = (double)grow[j * 3]; a[1] = (double)grow[j * 3 + 1]; a[2] = (double)grow[j * 3 + 2];
          b[0] = (double)grow[k * 3]; b[1] = (double)grow[k * 3 + 1]; b[2] = (double)grow[k * 3 + 2];
        }
        const double* P = &s_pG[(ti * A + n) * 9];
        double sum = 0.0;                                                   // :674 std::fill(...,0)
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) sum += ((a[l] * b[m]) * P[l * 3 + m]);   // :553 then :677-679, l-major
        if (!FIXUP) ok &= __builtin_amdgcn_class(sum, 0x100);
        acc[i] += FIXUP ? log(sum) : dmx_log2_fast(sum, s_log);                     // :683 / :709
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const int32_t q = q0 + t + i * kThreads;
    if (q < nAB) grid[(size_t)cell * nAB + q] = acc[i];
    else if (q < nacc) l00[(size_t)cell * A + (q - nAB)] = acc[i];
  }
  if (!FIXUP && !ok) flag_cell(flagged, cell);   // recomputed with ocml's log() by the FIXUP pass
  __syncthreads();                               // the next cell of this workgroup reuses the shared arrays
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// K2 for the default alpha grid size A = 2 (alpha[0] = singlet entry, alpha[1] = the doublet mixture).
// A cell is owned by TPC threads: TPC = 64 (V <= 16: one wavefront per cell, four independent cells per workgroup, no
// workgroup barrier in the loop) or TPC = 256 (V <= 64: one cell per workgroup).  Thread (j, kb) of the cell owns the
// 2*NK accumulators llksAB[j][kb*NK .. kb*NK+NK-1][0..1] in registers for the whole SNP range; it adds their log terms
// pair after pair, i.e. in the reference's ascending-SNP order.  Per tile of 32 covered pairs:
//   stage   the pairs' headers, then their genotype rows (float32, coalesced) into LDS;
//   phase 1 lane (pair ti, alpha n) of the cell's first wavefront: pG[n][3][3] with the shared-max renormalisation after
//           every read (:600-663) -> LDS; the same lane also forms the llks00 term of its (pair, alpha) (:699-709);
//   phase 2 every thread, for each pair in order: gpAB[l][m] = g_j[l]*g_k[m] (exact: float32 x float32 in binary64,
//           :553), the nine-term l-major sums for both alphas (:677-679), log, add (:683).
// log() arguments outside the normal positive range cannot occur for genuine likelihoods; if one does, the cell is
// flagged and recomputed by k_doublet_generic<FIXUP> with ocml's log().
// GD: the genotype rows are widened to binary64 once, when they are staged (a conversion per element and tile instead of one per
// use in phase 2); the LDS holds them as doubles.
// CHK = false drops the per-term argument-class test of phase 2 (a v_cmp_class_f64 per log): launched only when every genotype row was
// found finite, non-negative and not vanishing (k_check_geno) — then every phase-2 sum is >= max_l g_j[l] * (1e-6 / (1 + 1e-6)) *
// max_m g_k[m] > 2^-830, a normal positive number, and the test cannot fire.
// TP: covered pairs per tile (32; 16 or 8 on panels of more than ~180 samples, whose 32 staged genotype rows would leave one workgroup per CU)
// (the 64-thread-cell forms run three workgroups of four cells per CU = three wavefronts per SIMD: bounded to their 168 registers — left unbounded the
//  compiler's count moved from 158 to 246 with an unrelated edit of phase 1 and cfg5 STRICT lost a wavefront per SIMD, 144 -> 168 ms)
// SYMU (round 6, k_doublet_a2u below; V = 32 on 256 threads or 16 on 64, default grid): phase 2 over UNORDERED pairs — thread t owns the pairs {j, (j + d) % V} of units u = t
// and t + TPC (d = 1 + u / V, j = u % V; d = V/2 from j < V/2 only: 496 of 512 slots at V = 32, 120 of 128 at 16) with the four accumulators [j][k][0..1],
// [k][j][0..1] each: eight per thread, as before.
template <int TPC, int NK, int MINW, bool GD, bool CHK, int TP, bool SYMU, int MIR = 0>
__device__ __forceinline__ void a2_body(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                         const double* __restrict__ gp0, const double* __restrict__ tabs,
                                                         const double* __restrict__ alpha,
                                                         const int32_t* __restrict__ sched, int32_t V, int32_t GS,
                                                         double* __restrict__ grid, double* __restrict__ l00,
                                                         uint8_t* __restrict__ flagged, const double* __restrict__ pfin, const double* __restrict__ pseed) {
  static_assert(!SYMU || ((TPC == 256 || TPC == 64) && NK == 4 && !CHK), "symmetric ownership: 32 samples on 256 threads or 16 on 64, eight accumulators per thread, provably safe rows");
  constexpr int kUV = TPC == 256 ? 32 : 16, kUSh = kUV == 32 ? 5 : 4;       // SYMU: the panel (V (V - 1) / 2 unordered pairs on 2 TPC slots) and log2 of it
  // pfin (round 6; NULL unless the grid is {0, 0.5} and the pileup shallow): k_build_certify_finals' table of finished phase-1 values;
  // pseed (NULL unless the grid is {0, 0.5}): k_build_certify_seeds' table — on that grid the tiles that walk the read loop walk it in the five-value form
  // (alpha 0.5's five distinct mixing weights, alpha 0's three: entries of equal weight go through identical operations, so the nine values are these,
  // repeated) from the state after a pair's first one or two reads
  constexpr int A = 2;
  static_assert(TP == 32 || TP == 16 || TP == 8, "phase 1 runs on the first 2 * TP lanes of the cell's first wavefront");
  constexpr int CPW = kThreads / TPC;            // cells per workgroup
  constexpr int T00 = TP + 2;
#define DMX_K2_SYNC() do { if (TPC == 64) { DMX_WAVE_LDS_ORDER(); } else { __syncthreads(); } } while (0)
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_tab[kTab2];
  __shared__ double s_w[2][18];                  // mixing weights of :613 per alpha: [n][0..8] = p (ALT), [n][9..17] = 1 - p; in LDS so
                                                 // that they occupy registers only while phase 1 runs (36 VGPRs otherwise)
  const double* s_log = s_tab + kLut2;
  const int t = threadIdx.x;
  stage_k2_tables(s_tab, tabs, t, kThreads);
  if (t < 18) {
    const int n = t / 9, l = (t % 9) / 3, m = t % 3;
    const double p = 0.5 * l + (m - l) * 0.5 * alpha[n];
    s_w[n][t % 9] = p;
    s_w[n][9 + t % 9] = 1.0 - p;
  }
  __syncthreads();

  const int cw = t / TPC, tid = t % TPC;         // cell slot inside the workgroup, thread inside the cell
  // per-cell LDS regions
  using g_t = typename std::conditional<GD, double, float>::type;
  const size_t cell_bytes = (size_t)TP * 18 * 8 + (size_t)TP * GS * sizeof(g_t) + 2 * T00 * 8 + TP * (4 + 4 + 8);
  unsigned char* base = s_raw + (size_t)cw * cell_bytes;
  double* s_pG = (double*)base;                                  // [TP][2][9]
  g_t* s_g = (g_t*)(base + (size_t)TP * 18 * 8);                 // [TP][GS]   genotype rows of the tile's SNPs
  double* s_t00 = (double*)((unsigned char*)s_g + (size_t)TP * GS * sizeof(g_t));   // [2][T00]   llks00 terms
  int64_t* s_off = (int64_t*)(s_t00 + 2 * T00);                  // [TP]
  int32_t* s_snp = (int32_t*)(s_off + TP);                       // [TP]
  uint32_t* s_cnt = (uint32_t*)(s_snp + TP);                     // [TP]

  const int slot = blockIdx.x * CPW + cw;
  if (TPC == 64 && slot >= pv.B) return;         // whole wavefront idle (no workgroup barriers below in this mode)
  const bool cell_ok = slot < pv.B;
  const int32_t cell = cell_ok ? sched[slot] : 0;
  const int64_t p_beg = cell_ok ? pv.cell_pair_off[cell] : 0;
  const int64_t np = cell_ok ? pv.cell_pair_off[cell + 1] - p_beg : 0;
  int64_t rd_base = cell_ok ? pv.cell_read_off[cell] : 0;

  // phase-2 identity.  A workgroup covers JS = TPC / KB rows j of the cell's grid; panels with more rows than that are cut
  // into j-slabs, one workgroup (blockIdx.y) per slab, each repeating the cheap phases 0-1 for itself.
  const int KB = (V + NK - 1) / NK;              // k-blocks per j
  const int JS = TPC / KB;
  const int jl = tid / KB, kb = tid % KB;
  const int j = (int)blockIdx.y * JS + jl;
  const bool owner = jl < JS && j < V;
  double acc[NK][A];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) { acc[kk][0] = 0.0; acc[kk][1] = 0.0; }
  bool ok = true;
  const DmxLogPins lk = dmx_log_pins();
  int uj[2] = {0, 0}, uk[2] = {0, 0};            // SYMU: the thread's two unordered pairs; acc[2 su] = [j][k][0..1], acc[2 su + 1] = [k][j][0..1]
  if constexpr (SYMU) {
#pragma unroll
    for (int su = 0; su < 2; ++su) { const int u = tid + TPC * su; uj[su] = u & (kUV - 1); uk[su] = (uj[su] + 1 + (u >> kUSh)) & (kUV - 1); }
  }
  // SYMU: where the thread's rows start inside a staged genotype row, formed once (both units have the same j: TPC is a multiple of the panel)
  const g_t* const ga = s_g + uj[0] * 3;
  const g_t* const gb[2] = {s_g + uk[0] * 3, s_g + uk[1] * 3};
  // phase-1 identity (first wavefront of the cell): pair ti1, alpha n1; mixing weights of :613
  const int ti1 = tid >> 1, n1 = tid & 1;
  double acc00 = 0.0;                            // lane n1 == tid < 2 owns llks00[n]
  const int row_len = V * 3;

  for (int64_t tbase = 0; tbase < np; tbase += TP) {
    const int tp = (int)min((int64_t)TP, np - tbase);
    // ---- headers of the tile's pairs (first 32 lanes of the cell)
    load_tile_headers<TP>(pv, nrd_width, p_beg, tbase, tp, tid, rd_base, s_cnt, s_off, s_snp);
    DMX_K2_SYNC();
    rd_base = s_off[tp - 1] + (int64_t)s_cnt[tp - 1];
    // ---- genotype rows -> LDS (coalesced along the row)
    stage_geno_rows<TPC>(g, s_snp, tp, tid, row_len, GS, s_g);
    // ---- phase 1
    if (tid < 2 * TP) {
      const bool on = ti1 < tp;
      const uint32_t cnt = on ? s_cnt[ti1] : 0u;
      const int64_t off = on ? s_off[ti1] : 0;
      const uint32_t rd4 = load_rd4(pv, off, cnt);       // the first four read bytes in one load (one dependent latency instead of four)
      // Round 6 (default grid {0, 0.5}): pairs of up to three tabled reads take their finished values from the table — alpha 0.5's five distinct ones
      // q[l + m], alpha 0's three q[l]: entries of equal mixing weight go through identical operations, so the nine of the loop below repeat them bit for
      // bit — and the loop and the +1e-6 renormalisation run only in tiles with a deeper pair (wave-uniform branch); see k_doublet_sym.
      // (a tile with a deeper pair runs the loop for ALL its lanes, as before: no merge of the two sources, no register held across the loop)
      double vf[9];
      const int32_t fi = pfin ? certify_final_index(cnt, rd4) : -1;
      if (!__any(fi < 0)) {
        const double* fp = pfin + (size_t)fi * kCFinStride + (n1 ? 0 : 5);
        const double f0 = fp[0], f1 = fp[1], f2 = fp[2], f3 = n1 ? fp[3] : 0.0, f4 = n1 ? fp[4] : 0.0;
        const double f5[5] = {f0, f1, f2, f3, f4};
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) vf[l * 3 + m] = n1 ? f5[l + m] : f5[l];
      } else if (pseed) {
        double q5[5], wA5[5], wR5[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {                // the five-value form's weights: alpha 0.5: p = 0.25 (l + m), slot l + m; alpha 0: p = 0.5 l, slots 0..2 (3, 4 repeat 2)
          const int l = n1 ? (q > 2 ? 2 : q) : min(q, 2), m = n1 ? q - l : 0;
          const double p = 0.5 * l + (m - l) * 0.5 * (n1 ? 0.5 : 0.0);
          wA5[q] = p;
          wR5[q] = 1.0 - p;
        }
        certify_pair_values<5, false>(pv, cnt, off, rd4, s_tab, wA5, wR5, n1, q5, pseed);
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) vf[l * 3 + m] = n1 ? q5[l + m] : q5[l];
      } else {
        double wA[9], wR[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) { wA[i] = s_w[n1][i]; wR[i] = s_w[n1][9 + i]; }
        certify_pair_values<9, false, 2, true>(pv, cnt, off, rd4, s_tab, wA, wR, n1, vf);
      }
      if (on)
        ok &= llks00_term(gp0, s_snp[ti1], [&](int l, int m) { const double v = vf[l * 3 + m]; s_pG[(ti1 * 2 + n1) * 9 + l * 3 + m] = v; return v; },
                    s_log, &s_t00[n1 * T00 + ti1]);
    }
    DMX_K2_SYNC();
    // ---- llks00: lane n < 2 of the cell adds its alpha's terms in pair order
    if (tid < 2) {
      const double* row = &s_t00[tid * T00];
      if (tp == TP) {                              // loads first (LDS latency paid once), then the ordered adds
        double2 v[TP / 2];
#pragma unroll
        for (int i = 0; i < TP / 2; ++i) v[i] = *reinterpret_cast<const double2*>(&row[2 * i]);
#pragma unroll
        for (int i = 0; i < TP / 2; ++i) { acc00 += v[i].x; acc00 += v[i].y; }
      } else {
        for (int i = 0; i < tp; ++i) acc00 += row[i];
      }
    }
    // ---- phase 2
    if constexpr (SYMU) {
      // At alpha 0.5 the mixture is symmetric — pG[1][l][m] == pG[1][m][l] bit for bit (equal mixing weights go through identical operations) — so the
      // nine terms (g_k[l] g_j[m]) pG[1][l][m] of entry [k][j] are entry [j][k]'s T[l][m] = (g_j[l] g_k[m]) pG[1][l][m], transposed: the reference adds them
      // l-major for [j][k] and, seen from [j][k]'s indices, m-major for [k][j].  The owner of both forms the exact products E and the terms T once: 36
      // multiplies per unordered pair instead of 54; the 32 adds, the four logs and the four accumulator adds are the reference's, on its operands, in its order.
      // Order inside a pair: a unit forms its four sums, then requests the four table entries of their logs TOGETHER (dmx_log2_request_fast) and runs the four
      // second halves behind one LDS wait (the logs one after the other left each entry's round trip exposed: ten waits per pair).  Unit 1's k row is
      // requested behind unit 0's table entries, the next pair's values and rows once unit 1's entries are in: every other LDS read of the loop travels while
      // logs are evaluated (three s_waitcnt lgkmcnt per pair, the one at the top of the loop for reads issued four logs earlier).
      // The tile's pair count is workgroup-uniform (wavefront-uniform for the one-wavefront cells): a scalar loop counter.
      const int tps = __builtin_amdgcn_readfirstlane(tp);
      double Q[3], P1[5];
      g_t ar[3], br[3];
      auto load_pair = [&](int pi) {
        const double* P = &s_pG[pi * 18];
        Q[0] = P[0]; Q[1] = P[3]; Q[2] = P[6];                               // pG[0][l][m] = q0[l]
        P1[0] = P[9]; P1[1] = P[10]; P1[2] = P[11]; P1[3] = P[14]; P1[4] = P[17];   // pG[1][l][m] = q1[l + m]
        const g_t* ra = &ga[pi * GS];
        const g_t* rb = &gb[0][pi * GS];
        ar[0] = ra[0]; ar[1] = ra[1]; ar[2] = ra[2];
        br[0] = rb[0]; br[1] = rb[1]; br[2] = rb[2];
      };
      load_pair(0);
      for (int ti = 0; ti < tps; ++ti) {
        const double a[3] = {(double)ar[0], (double)ar[1], (double)ar[2]};
#pragma unroll
        for (int su = 0; su < 2; ++su) {
          const double b[3] = {(double)br[0], (double)br[1], (double)br[2]};
          double E[3][3];
#pragma unroll
          for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int m = 0; m < 3; ++m) E[l][m] = a[l] * b[m];                  // :553 (exact) — shared by [j][k] and [k][j] at both alphas
          // [j][k][0]: l-major over (l, m) of (g_j[l] g_k[m]) q0[l]; [k][j][0]: of (g_k[l] g_j[m]) q0[l] = E[m][l] q0[l] (the first product initialises the sum)
          double s_jk0 = E[0][0] * Q[0], s_kj0 = E[0][0] * Q[0];
#pragma unroll
          for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int m = 0; m < 3; ++m) {
              if (l == 0 && m == 0) continue;
              s_jk0 += (E[l][m] * Q[l]);
              s_kj0 += (E[m][l] * Q[l]);
            }
#pragma unroll
          for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int m = 0; m < 3; ++m) E[l][m] = E[l][m] * P1[l + m];          // T: :677-679 at alpha 0.5 — [k][j]'s nine terms are these, transposed
          double s_jk1 = E[0][0], s_kj1 = E[0][0];
#pragma unroll
          for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int m = 0; m < 3; ++m) {
              if (l == 0 && m == 0) continue;
              s_jk1 += E[l][m];
              s_kj1 += E[m][l];
            }
          // MIR != 0 (k_doublet_a2u16; 2: its _mirror_fallback form, every mirror whole): s_jk1 and s_kj1 are a mirrored pair (dmx_log.hpp) — three table entries
          // per unit, [k][j]'s log from [j][k]'s entry, kd and w, settled behind the unit's guard test.  MIR == 0 (k_doublet_a2u<MINW>): four independent logs —
          // with the mirrored form that kernel spills four more registers at its 128.
          const DmxLog2Req r_jk0 = dmx_log2_request_fast(s_jk0, s_log), r_kj0 = dmx_log2_request_fast(s_kj0, s_log);
          DmxLog2Req r_jk1, r_kj1;
          DmxLog2MirrorReq r_1;
          if constexpr (MIR != 0) r_1 = dmx_log2_request_mirror_fast(s_jk1, s_kj1, s_log);
          else { r_jk1 = dmx_log2_request_fast(s_jk1, s_log); r_kj1 = dmx_log2_request_fast(s_kj1, s_log); }
          if (su == 0) {
            const g_t* rb = &gb[1][ti * GS];
            br[0] = rb[0]; br[1] = rb[1]; br[2] = rb[2];
          }
          __builtin_amdgcn_sched_barrier(0);                                   // requests first: nothing of the arithmetic below moves above them
          __builtin_amdgcn_s_waitcnt(0xC07F);                                  // lgkmcnt(0): ONE wait for the unit's four entries (left alone: one per entry)
          __builtin_amdgcn_sched_barrier(0);                                   // (the wait has no operands: without this it sinks below the arithmetic)
          if (su == 1) {
            load_pair(min(ti + 1, tps - 1));                                   // (the tile's last pair requests itself again: nothing reads it)
            __builtin_amdgcn_sched_barrier(0);
          }
          acc[2 * su][0] += dmx_log2_finish_pinned(r_jk0, lk);                 // :683
          acc[2 * su + 1][0] += dmx_log2_finish_pinned(r_kj0, lk);
          if constexpr (MIR != 0) {
            double y_kj1;
            acc[2 * su][1] += dmx_log2_finish_mirror_pinned(r_1, lk, &y_kj1);
            if (dmx_log2_mirror_any_redo<MIR == 2>(r_1.guard)) y_kj1 = dmx_log2_mirror_settle<MIR == 2>(r_1.guard, r_1, y_kj1, s_log, lk);   // never taken in practice
            acc[2 * su + 1][1] += y_kj1;
          } else {
            acc[2 * su][1] += dmx_log2_finish_pinned(r_jk1, lk);
            acc[2 * su + 1][1] += dmx_log2_finish_pinned(r_kj1, lk);
          }
          __builtin_amdgcn_sched_barrier(0);                                   // one unit's logs at a time (register budget; without it: no faster)
        }
      }
    } else
    if (owner) {
      for (int ti = 0; ti < tp; ++ti) {
        const double* P = &s_pG[ti * 18];
        double P0[9], P1[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) { P0[i] = P[i]; P1[i] = P[9 + i]; }
        const g_t* gr = &s_g[ti * GS];
        const double a0 = (double)gr[j * 3], a1 = (double)gr[j * 3 + 1], a2 = (double)gr[j * 3 + 2];
        const double aj[3] = {a0, a1, a2};
#pragma unroll
        for (int kk = 0; kk < NK; ++kk) {
          const int k = min(kb * NK + kk, V - 1);
          const double b0 = (double)gr[k * 3], b1 = (double)gr[k * 3 + 1], b2 = (double)gr[k * 3 + 2];
          const double bk[3] = {b0, b1, b2};
          // :674-679, l-major.  The reference starts from 0 and adds nine products; 0 + x is x for these non-negative
          // products (no -0 can occur), so the first product initialises the sum: same bits, one add fewer per term.
          double s0 = (aj[0] * bk[0]) * P0[0], s1 = (aj[0] * bk[0]) * P1[0];
#pragma unroll
          for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int m = 0; m < 3; ++m) {
              if (l == 0 && m == 0) continue;
              const double gp = aj[l] * bk[m];                                // :553 (exact)
              s0 += (gp * P0[l * 3 + m]);                                     // alpha 0
              s1 += (gp * P1[l * 3 + m]);                                     // alpha 1
            }
          if (CHK) ok &= __builtin_amdgcn_class(s0, 0x100) && __builtin_amdgcn_class(s1, 0x100);
          acc[kk][0] += dmx_log2_fast_pinned(s0, s_log, lk);                   // :683
          acc[kk][1] += dmx_log2_fast_pinned(s1, s_log, lk);
        }
      }
    }
    DMX_K2_SYNC();
  }
  if (cell_ok) {
    if constexpr (SYMU) {
#pragma unroll
      for (int su = 0; su < 2; ++su) {
        const int u = tid + TPC * su, d = 1 + (u >> kUSh);
        if (d < kUV / 2 || (d == kUV / 2 && uj[su] < kUV / 2)) {   // d = V/2 is reached from both sides: the j < V/2 thread stores; units beyond the last pair do not exist
          double* o = grid + (((size_t)cell * V + uj[su]) * V + uk[su]) * A;
          o[0] = acc[2 * su][0]; o[1] = acc[2 * su][1];
          double* o2 = grid + (((size_t)cell * V + uk[su]) * V + uj[su]) * A;
          o2[0] = acc[2 * su + 1][0]; o2[1] = acc[2 * su + 1][1];
        }
      }
    } else
    if (owner) {
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        const int k = kb * NK + kk;
        if (k < V) {
          double* o = grid + (((size_t)cell * V + j) * V + k) * A;
          o[0] = acc[kk][0]; o[1] = acc[kk][1];
        }
      }
    }
    if (tid < 2 && blockIdx.y == 0) l00[(size_t)cell * A + tid] = acc00;
    if (!ok) flag_cell(flagged, cell);
  }
#undef DMX_K2_SYNC
}
template <int TPC, int NK, int MINW = 1, bool GD = false, bool CHK = true, int TP = 32>
__global__ __launch_bounds__(kThreads, (MINW == 1 && TPC == 64) ? 3 : MINW) void k_doublet_a2(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                         const double* __restrict__ gp0, const double* __restrict__ tabs,
                                                         const double* __restrict__ alpha,
                                                         const int32_t* __restrict__ sched, int32_t V, int32_t GS,
                                                         double* __restrict__ grid, double* __restrict__ l00,
                                                         uint8_t* __restrict__ flagged, const double* __restrict__ pfin, const double* __restrict__ pseed) {
  a2_body<TPC, NK, MINW, GD, CHK, TP, false>(pv, nrd_width, g, gp0, tabs, alpha, sched, V, GS, grid, l00, flagged, pfin, pseed);
}
// k_doublet_a2 over unordered pairs (STRICT, default grid, 32 soft-field samples: cfg3 — the headline): everything of k_doublet_a2<256,4,4,GD,noCHK> but phase 2's
// ownership (SYMU above).  The 32 diagonal entries [j][j][n] are not its: k_doublet_a2s<.., 0> (one wavefront per barcode) adds them behind it.
template <int MINW>
__global__ __launch_bounds__(kThreads, MINW) void k_doublet_a2u(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                          const double* __restrict__ gp0, const double* __restrict__ tabs,
                                                          const double* __restrict__ alpha,
                                                          const int32_t* __restrict__ sched, int32_t V, int32_t GS,
                                                          double* __restrict__ grid, double* __restrict__ l00,
                                                          uint8_t* __restrict__ flagged, const double* __restrict__ pfin, const double* __restrict__ pseed) {
  a2_body<256, 4, MINW, true, false, 32, true>(pv, nrd_width, g, gp0, tabs, alpha, sched, V, GS, grid, l00, flagged, pfin, pseed);
}
// ... and for 16 samples (cfg5): k_doublet_a2<64,4,1,noCHK>'s kernel — 64 threads per barcode, four barcodes per workgroup, three wavefronts per SIMD
__global__ __launch_bounds__(kThreads, 3) void k_doublet_a2u16(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                          const double* __restrict__ gp0, const double* __restrict__ tabs,
                                                          const double* __restrict__ alpha,
                                                          const int32_t* __restrict__ sched, int32_t V, int32_t GS,
                                                          double* __restrict__ grid, double* __restrict__ l00,
                                                          uint8_t* __restrict__ flagged, const double* __restrict__ pfin, const double* __restrict__ pseed) {
  a2_body<64, 4, 1, false, false, 32, true, 1>(pv, nrd_width, g, gp0, tabs, alpha, sched, V, GS, grid, l00, flagged, pfin, pseed);
}
// ... with every mirrored log on its slow path (tests only: DMX_EXPERIMENTS=1 DMX_A2U_MIRROR_FALLBACK=1)
__global__ __launch_bounds__(kThreads, 3) void k_doublet_a2u16_mirror_fallback(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                          const double* __restrict__ gp0, const double* __restrict__ tabs,
                                                          const double* __restrict__ alpha,
                                                          const int32_t* __restrict__ sched, int32_t V, int32_t GS,
                                                          double* __restrict__ grid, double* __restrict__ l00,
                                                          uint8_t* __restrict__ flagged, const double* __restrict__ pfin, const double* __restrict__ pseed) {
  a2_body<64, 4, 1, false, false, 32, true, 2>(pv, nrd_width, g, gp0, tabs, alpha, sched, V, GS, grid, l00, flagged, pfin, pseed);
}

// k_doublet_a2u for TWO barcodes per workgroup (32 samples, STRICT, default grid, provably safe rows, DENSE pileups: cfg3 — the headline).  The exact products
// E[l][m] = g_j[l] g_k[m] (:553) depend on the SNP and the sample pair, not on the barcode, and pair p of every barcode of a dense pileup is SNP p: two barcodes
// that walk their pairs in lockstep need E once.  Workgroup (x, y) owns the barcodes of schedule slots 2x and 2x + 1 and slab y of the 496 unordered pairs: thread
// tid owns ONE unit u = tid + 256 y (k_doublet_a2u's mapping: j = u % 32, d = 1 + u / 32, k = (j + d) % 32, d = 16 from j < 16 only) for BOTH barcodes — eight
// accumulators, as there.  Everything else stays per barcode with the reference's operands in the reference's order: 209 FP64 instructions per pair where
// k_doublet_a2u's thread spends 218 on its two units of one barcode.  (207 since a barcode's two alpha-0.5 logs share one front end: the mirrored log, dmx_log.hpp.)
// Per tile of 32 pairs: headers of both barcodes (the first wavefront: lanes 0..31 barcode 0, 32..63 barcode 1; the SNP ids are the pair indices), the 32 rows
// staged ONCE as binary64, phase 1 on 128 lanes (wavefront = barcode, lane = (pair, alpha); the table / loop test is per wavefront) which leaves the EIGHT values
// phase 2 reads per (barcode, pair) — alpha 0.5's q1[0..4] | alpha 0's q0[0..2], k_doublet_diag's layout; the eighteen-value layout would not fit four
// workgroups per CU — and, in slab 0 only, the llks00 terms.  A lone last barcode (odd B) is walked twice; the second copy stores nothing.
// Every barcode of a dense pileup has the same pair count (checked when the pileup is set), so the tile loop and its barriers are workgroup-uniform.
// DIAG16: slab 1's last sixteen slots (u = 496..511), which otherwise repeat units that exist, take k = j for j = 16..31: E = g_j x g_j, and the unit's l-major
// [j][k] sums are the diagonal entries [j][j][0..1] as the reference and k_doublet_diag form them (the [k][j] sums of such a unit are dropped); k_doublet_diag_lo
// behind the kernel then owns j = 0..15 only.
// The kernel is a form of the unordered-pair kernel and is named so: k_doublet_a2u<k_doublet_a2u2> (the shipped form, DIAG16) and
// k_doublet_a2u<k_doublet_a2u2_whole_diag_behind> are what dmx_engine_kernel_names and the profiler report.
struct k_doublet_a2u2 { static constexpr bool diag16 = true; };
struct k_doublet_a2u2_whole_diag_behind { static constexpr bool diag16 = false; };
// MFB (k_doublet_a2u<k_doublet_a2u2_mirror_fallback>, tests only): the mirrored logs' guard is compile-time false, every [k][j] alpha-0.5 log takes the slow path
struct k_doublet_a2u2_mirror_fallback { static constexpr bool diag16 = true, mirror_fallback = true; };
template <bool DIAG16, bool MFB = false>
__device__ __forceinline__ void a2u2_body(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                         const double* __restrict__ gp0, const double* __restrict__ tabs,
                                                         const double* __restrict__ alpha, const int32_t* __restrict__ sched,
                                                         double* __restrict__ grid, double* __restrict__ l00,
                                                         uint8_t* __restrict__ flagged, const double* __restrict__ pfin, const double* __restrict__ pseed) {
  constexpr int V = 32, A = 2, TP = 32, T00 = TP + 2, GS = 3 * V, row_len = 3 * V;
  __shared__ double s_tab[kTab2];
  __shared__ double s_w[2][18];                  // the nine-value loop's mixing weights (a2_body's)
  __shared__ __attribute__((aligned(16))) double s_q[2][TP][8];          // [barcode][pair]: q1[0..4] (alpha 0.5, index l + m) | q0[0..2] (alpha 0, index l)
  __shared__ __attribute__((aligned(16))) double s_g[TP * GS];           // genotype rows of the tile's SNPs, binary64
  __shared__ __attribute__((aligned(16))) double s_t00[2][2][T00];       // [barcode][alpha]: llks00 terms (slab 0)
  __shared__ int64_t s_off[2][TP];
  __shared__ int32_t s_snp[2][TP];               // (the same ids twice: each header lane group publishes its own copy)
  __shared__ uint32_t s_cnt[2][TP];
  const double* s_log = s_tab + kLut2;
  const int tid = threadIdx.x;
  stage_k2_tables(s_tab, tabs, tid, kThreads);
  if (tid < 18) {
    const int n = tid / 9, l = (tid % 9) / 3, m = tid % 3;
    const double p = 0.5 * l + (m - l) * 0.5 * alpha[n];
    s_w[n][tid % 9] = p;
    s_w[n][9 + tid % 9] = 1.0 - p;
  }
  __syncthreads();

  const int slot0 = 2 * (int)blockIdx.x;         // < B by the launch grid
  const bool two = slot0 + 1 < pv.B;             // odd B: the last workgroup's second barcode does not exist — it walks the first one again and stores nothing
  const bool slab0 = blockIdx.y == 0;
  // header lanes (tid < 64: barcode hb, pair hl of the tile) and phase-1 lanes (tid < 128: barcode bb, pair ti1, alpha n1)
  const int hb = (tid >> 5) & 1, hl = tid & 31;
  const int bb = (tid >> 6) & 1, ti1 = (tid & 63) >> 1, n1 = tid & 1;
  const int32_t cell0 = sched[slot0], cell1 = two ? sched[slot0 + 1] : cell0;
  const int32_t cell_h = hb ? cell1 : cell0;
  const int64_t p_beg = pv.cell_pair_off[cell_h];
  int64_t rd_base = pv.cell_read_off[cell_h];
  const int np = (int)(pv.cell_pair_off[cell0 + 1] - pv.cell_pair_off[cell0]);   // the pileup's common pair count: the same value in every thread

  const int u = tid + kThreads * (int)blockIdx.y, uj = u & 31, ud = 1 + (u >> 5);
  const bool udiag = DIAG16 && u >= 496;         // (j = 16..31)
  const int uk = udiag ? uj : (uj + ud) & 31;
  const double* const ga = s_g + uj * 3;
  const double* const gb = s_g + uk * 3;
  double acc[2][4];                              // [barcode]: [j][k][0], [k][j][0], [j][k][1], [k][j][1]
#pragma unroll
  for (int c = 0; c < 2; ++c) { acc[c][0] = 0.0; acc[c][1] = 0.0; acc[c][2] = 0.0; acc[c][3] = 0.0; }
  bool ok = true;
  double acc00 = 0.0;                            // slab 0, tid < 4: llks00[alpha tid & 1] of barcode tid >> 1
  const DmxLogPins lk = dmx_log_pins();

  for (int tbase = 0; tbase < np; tbase += TP) {
    const int tp = min(TP, np - tbase);
    // ---- headers of the tile's pairs, both barcodes
    if (tid < 64) load_tile_headers<TP>(pv, nrd_width, p_beg, (int64_t)tbase, tp, hl, rd_base, s_cnt[hb], s_off[hb], s_snp[hb]);
    __syncthreads();
    if (tid < 64) rd_base = s_off[hb][tp - 1] + (int64_t)s_cnt[hb][tp - 1];
    // ---- genotype rows -> LDS, once for both barcodes
    stage_geno_rows<kThreads>(g, s_snp[0], tp, tid, row_len, GS, s_g);
    // ---- phase 1
    if (tid < 4 * TP) {
      const bool on = ti1 < tp;
      const uint32_t cnt = on ? s_cnt[bb][ti1] : 0u;
      const int64_t off = on ? s_off[bb][ti1] : 0;
      const uint32_t rd4 = load_rd4(pv, off, cnt);
      double vf[9];                                // (a2_body's three sources, as there)
      const int32_t fi = pfin ? certify_final_index(cnt, rd4) : -1;
      if (!__any(fi < 0)) {
        const double* fp = pfin + (size_t)fi * kCFinStride + (n1 ? 0 : 5);
        const double f0 = fp[0], f1 = fp[1], f2 = fp[2], f3 = n1 ? fp[3] : 0.0, f4 = n1 ? fp[4] : 0.0;
        const double f5[5] = {f0, f1, f2, f3, f4};
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) vf[l * 3 + m] = n1 ? f5[l + m] : f5[l];
      } else if (pseed) {
        double q5[5], wA5[5], wR5[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
          const int l = n1 ? (q > 2 ? 2 : q) : min(q, 2), m = n1 ? q - l : 0;
          const double p = 0.5 * l + (m - l) * 0.5 * (n1 ? 0.5 : 0.0);
          wA5[q] = p;
          wR5[q] = 1.0 - p;
        }
        certify_pair_values<5, false>(pv, cnt, off, rd4, s_tab, wA5, wR5, n1, q5, pseed);
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) vf[l * 3 + m] = n1 ? q5[l + m] : q5[l];
      } else {
        double wA[9], wR[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) { wA[i] = s_w[n1][i]; wR[i] = s_w[n1][9 + i]; }
        certify_pair_values<9, false, 2, true>(pv, cnt, off, rd4, s_tab, wA, wR, n1, vf);
      }
      if (on) {
        double* q = &s_q[bb][ti1][0];
        if (n1) { q[0] = vf[0]; q[1] = vf[1]; q[2] = vf[2]; q[3] = vf[5]; q[4] = vf[8]; }   // pG[1][l][m] = q1[l + m]
        else { q[5] = vf[0]; q[6] = vf[3]; q[7] = vf[6]; }                                  // pG[0][l][m] = q0[l]
        if (slab0)                                 // (workgroup-uniform) the llks00 term from the nine values in registers
          ok &= llks00_term(gp0, s_snp[bb][ti1], [&](int l, int m) { return vf[l * 3 + m]; }, s_log, &s_t00[bb][n1][ti1]);
      }
    }
    __syncthreads();
    // ---- llks00 (slab 0): lane (barcode, alpha) adds its terms in pair order
    if (slab0 && tid < 4) {
      const double* row = &s_t00[tid >> 1][tid & 1][0];
      if (tp == TP) {
        double2 v[TP / 2];
#pragma unroll
        for (int i = 0; i < TP / 2; ++i) v[i] = *reinterpret_cast<const double2*>(&row[2 * i]);
#pragma unroll
        for (int i = 0; i < TP / 2; ++i) { acc00 += v[i].x; acc00 += v[i].y; }
      } else {
        for (int i = 0; i < tp; ++i) acc00 += row[i];
      }
    }
    // ---- phase 2: the thread's unit, both barcodes.  E once; per barcode k_doublet_a2u's sums (a2_body, SYMU), logs and adds on its operands in its order.
    // Barcode 1's alpha-0.5 terms T' go to fresh registers, barcode 0's T replace E.  The eight logs run in two batches of four (a barcode each): four table
    // entries requested together, one wait, four second halves; the next pair's rows and q values are requested while logs are evaluated.
    // A barcode's two alpha-0.5 sums s_jk1 and s_kj1 are a mirrored pair (dmx_log.hpp): three table entries per barcode, [k][j]'s log from [j][k]'s entry, kd and w.
    // Its value is held until the iteration's one guard test (both barcodes' guard words, wave-uniform, never taken in practice) and added behind it.
    {
      const int tps = __builtin_amdgcn_readfirstlane(tp);
      double Q[2][3], P1[2][5], ar[3], br[3];
      auto load_pair = [&](int pi) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const double* q = &s_q[c][pi][0];
          P1[c][0] = q[0]; P1[c][1] = q[1]; P1[c][2] = q[2]; P1[c][3] = q[3]; P1[c][4] = q[4];
          Q[c][0] = q[5]; Q[c][1] = q[6]; Q[c][2] = q[7];
        }
        const double* ra = &ga[pi * GS];
        const double* rb = &gb[pi * GS];
        ar[0] = ra[0]; ar[1] = ra[1]; ar[2] = ra[2];
        br[0] = rb[0]; br[1] = rb[1]; br[2] = rb[2];
      };
      load_pair(0);
      for (int ti = 0; ti < tps; ++ti) {
        double E[3][3], T1[3][3];
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) E[l][m] = ar[l] * br[m];                  // :553 (exact) — shared by [j][k] and [k][j], both alphas, BOTH barcodes
        // [j][k][0]: l-major over (l, m) of (g_j[l] g_k[m]) q0[l]; [k][j][0]: of (g_k[l] g_j[m]) q0[l] = E[m][l] q0[l] (the first product initialises the sum)
        double s_jk0[2], s_kj0[2], s_jk1[2], s_kj1[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          s_jk0[c] = E[0][0] * Q[c][0]; s_kj0[c] = E[0][0] * Q[c][0];
#pragma unroll
          for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int m = 0; m < 3; ++m) {
              if (l == 0 && m == 0) continue;
              s_jk0[c] += (E[l][m] * Q[c][l]);
              s_kj0[c] += (E[m][l] * Q[c][l]);
            }
        }
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            T1[l][m] = E[l][m] * P1[1][l + m];                                   // T': barcode 1's terms (:677-679 at alpha 0.5), fresh registers
            E[l][m] = E[l][m] * P1[0][l + m];                                    // T: barcode 0's, in place
          }
        s_jk1[0] = E[0][0]; s_kj1[0] = E[0][0];
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            if (l == 0 && m == 0) continue;
            s_jk1[0] += E[l][m];
            s_kj1[0] += E[m][l];
          }
        // barcode 0's four table entries travel while barcode 1's alpha-0.5 sums are formed
        const DmxLog2Req a_jk0 = dmx_log2_request_fast(s_jk0[0], s_log), a_kj0 = dmx_log2_request_fast(s_kj0[0], s_log);
        const DmxLog2MirrorReq a_1 = dmx_log2_request_mirror_fast(s_jk1[0], s_kj1[0], s_log);
        __builtin_amdgcn_sched_barrier(0);                                     // requests first: nothing of the arithmetic below moves above them
        s_jk1[1] = T1[0][0]; s_kj1[1] = T1[0][0];
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            if (l == 0 && m == 0) continue;
            s_jk1[1] += T1[l][m];
            s_kj1[1] += T1[m][l];
          }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0xC07F);                                    // lgkmcnt(0): ONE wait for the barcode's four entries
        __builtin_amdgcn_sched_barrier(0);                                     // (the wait has no operands: without this it sinks below the arithmetic)
        // barcode 1's entries, the next pair's q values and rows: every other LDS read of the pair travels while barcode 0's logs are evaluated
        const DmxLog2Req b_jk0 = dmx_log2_request_fast(s_jk0[1], s_log), b_kj0 = dmx_log2_request_fast(s_kj0[1], s_log);
        const DmxLog2MirrorReq b_1 = dmx_log2_request_mirror_fast(s_jk1[1], s_kj1[1], s_log);
        const uint32_t mguard = a_1.guard | b_1.guard;
        load_pair(min(ti + 1, tps - 1));                                       // (the tile's last pair requests itself again: nothing reads it)
        __builtin_amdgcn_sched_barrier(0);
        acc[0][0] += dmx_log2_finish_pinned(a_jk0, lk);                        // :683
        acc[0][1] += dmx_log2_finish_pinned(a_kj0, lk);
        double ya_kj1, yb_kj1;
        acc[0][2] += dmx_log2_finish_mirror_pinned(a_1, lk, &ya_kj1);
        asm volatile("" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(ya_kj1));      // barcode 0's logs stay in front of the second wait
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_sched_barrier(0);
        acc[1][0] += dmx_log2_finish_pinned(b_jk0, lk);
        acc[1][1] += dmx_log2_finish_pinned(b_kj0, lk);
        acc[1][2] += dmx_log2_finish_mirror_pinned(b_1, lk, &yb_kj1);
        if (dmx_log2_mirror_any_redo<MFB>(mguard)) {                           // out of line: the lanes whose guard failed evaluate their mirrors whole
          ya_kj1 = dmx_log2_mirror_settle<MFB>(mguard, a_1, ya_kj1, s_log, lk);
          yb_kj1 = dmx_log2_mirror_settle<MFB>(mguard, b_1, yb_kj1, s_log, lk);
        }
        acc[0][3] += ya_kj1;
        acc[1][3] += yb_kj1;
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();
  }
  if (ud < 16 || (ud == 16 && uj < 16) || udiag) {   // d = 16 is reached from both sides: the j < 16 thread stores; slab 1's last sixteen slots repeat units that exist, or hold a diagonal entry
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (c == 1 && !two) break;
      const int32_t cell = c ? cell1 : cell0;
      double* o = grid + (((size_t)cell * V + uj) * V + uk) * A;
      o[0] = acc[c][0]; o[1] = acc[c][2];
      if (!udiag) {
        double* o2 = grid + (((size_t)cell * V + uk) * V + uj) * A;
        o2[0] = acc[c][1]; o2[1] = acc[c][3];
      }
    }
  }
  if (slab0 && tid < 4 && (tid < 2 || two)) l00[(size_t)((tid >> 1) ? cell1 : cell0) * A + (tid & 1)] = acc00;
  if (!ok) flag_cell(flagged, bb ? cell1 : cell0);  // (phase-1 lanes of slab 0 only; a lone barcode's second copy flags the barcode itself)
}
template <class FORM, class = void> struct a2u2_mirror_fallback_of { static constexpr bool value = false; };
template <class FORM> struct a2u2_mirror_fallback_of<FORM, std::enable_if_t<FORM::mirror_fallback>> { static constexpr bool value = true; };
template <class FORM>                            // FORM: k_doublet_a2u2, k_doublet_a2u2_whole_diag_behind or k_doublet_a2u2_mirror_fallback (k_doublet_a2u<MINW> above is the one-barcode kernel)
__global__ __launch_bounds__(kThreads, 4) void k_doublet_a2u(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                         const double* __restrict__ gp0, const double* __restrict__ tabs,
                                                         const double* __restrict__ alpha, const int32_t* __restrict__ sched,
                                                         double* __restrict__ grid, double* __restrict__ l00,
                                                         uint8_t* __restrict__ flagged, const double* __restrict__ pfin, const double* __restrict__ pseed) {
  a2u2_body<FORM::diag16, a2u2_mirror_fallback_of<FORM>::value>(pv, nrd_width, g, gp0, tabs, alpha, sched, grid, l00, flagged, pfin, pseed);
}

// K2, A = 2, FAST mode (dmx_engine_config.mode = DMX_MODE_FAST): k_doublet_a2 with the bilinear factoring of SURVEY H3.  Not the
// reference's operation sequence inside a term (so not STRICT), but the same accumulation order; tests bound it by 1e-9.
template <int TPC, int NK>
__global__ __launch_bounds__(kThreads, 3) void k_doublet_a2f(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                         const double* __restrict__ gp0, const double* __restrict__ tabs,
                                                         const double* __restrict__ alpha,
                                                         const int32_t* __restrict__ sched, int32_t V, int32_t GS,
                                                         double* __restrict__ grid, double* __restrict__ l00,
                                                         uint8_t* __restrict__ flagged) {
  constexpr int A = 2, TP = 32;
  constexpr int CPW = kThreads / TPC;            // cells per workgroup
  constexpr int T00 = TP + 2;
#define DMX_K2_SYNC() do { if (TPC == 64) { DMX_WAVE_LDS_ORDER(); } else { __syncthreads(); } } while (0)
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_tab[kTab2];
  const double* s_log = s_tab + kLut2;
  const int t = threadIdx.x;
  stage_k2_tables(s_tab, tabs, t, kThreads);
  __syncthreads();

  const int cw = t / TPC, tid = t % TPC;         // cell slot inside the workgroup, thread inside the cell
  // per-cell LDS regions
  constexpr bool SHARE = TPC > 64;               // one-wavefront cells (V <= 16) form u in registers: no LDS tile, no extra syncs
  constexpr int SUB = 8;                         // pairs per u sub-tile
  const int VU = V;                              // u row: [alpha][k][4 doubles] (4th pads the 3 to 32 bytes)
  const size_t cell_bytes = (size_t)TP * 18 * 8 + (size_t)TP * GS * 4 + 2 * T00 * 8 + TP * (4 + 4 + 8) + (SHARE ? (size_t)SUB * 2 * VU * 32 : 0);
  unsigned char* base = s_raw + (size_t)cw * cell_bytes;
  double* s_pG = (double*)base;                                  // [TP][2][9]
  float* s_g = (float*)(base + (size_t)TP * 18 * 8);             // [TP][GS]   genotype rows of the tile's SNPs
  double* s_t00 = (double*)((unsigned char*)s_g + (size_t)TP * GS * 4);   // [2][T00]   llks00 terms
  int64_t* s_off = (int64_t*)(s_t00 + 2 * T00);                  // [TP]
  int32_t* s_snp = (int32_t*)(s_off + TP);                       // [TP]
  uint32_t* s_cnt = (uint32_t*)(s_snp + TP);                     // [TP]
  double* s_u = (double*)(s_cnt + TP);                           // [SUB][2][V][4]   u[l] = sum_m pG[n][l][m] * g_k[m]

  const int slot = blockIdx.x * CPW + cw;
  if (TPC == 64 && slot >= pv.B) return;         // whole wavefront idle (no workgroup barriers below in this mode)
  const bool cell_ok = slot < pv.B;
  const int32_t cell = cell_ok ? sched[slot] : 0;
  const int64_t p_beg = cell_ok ? pv.cell_pair_off[cell] : 0;
  const int64_t np = cell_ok ? pv.cell_pair_off[cell + 1] - p_beg : 0;
  int64_t rd_base = cell_ok ? pv.cell_read_off[cell] : 0;

  // phase-2 identity.  A workgroup covers JS = TPC / KB rows j of the cell's grid; panels with more rows than that are cut
  // into j-slabs, one workgroup (blockIdx.y) per slab, each repeating the cheap phases 0-1 for itself.
  const int KB = (V + NK - 1) / NK;              // k-blocks per j
  const int JS = TPC / KB;
  const int jl = tid / KB, kb = tid % KB;
  const int j = (int)blockIdx.y * JS + jl;
  const bool owner = jl < JS && j < V;
  double acc[NK][A];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) { acc[kk][0] = 0.0; acc[kk][1] = 0.0; }
  bool ok = true;
  const DmxLogPins lk = dmx_log_pins();
  // phase-1 identity (first wavefront of the cell): pair ti1, alpha n1; mixing weights of :613
  const int ti1 = tid >> 1, n1 = tid & 1;
  double wA[9], wR[9];
  {
    const double al = alpha[n1];
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const double p = 0.5 * l + (m - l) * 0.5 * al;
        wA[l * 3 + m] = p;
        wR[l * 3 + m] = 1.0 - p;
      }
  }
  double acc00 = 0.0;                            // lane n1 == tid < 2 owns llks00[n]
  const int row_len = V * 3;

  for (int64_t tbase = 0; tbase < np; tbase += TP) {
    const int tp = (int)min((int64_t)TP, np - tbase);
    // ---- headers of the tile's pairs (first 32 lanes of the cell)
    load_tile_headers<TP>(pv, nrd_width, p_beg, tbase, tp, tid, rd_base, s_cnt, s_off, s_snp);
    DMX_K2_SYNC();
    rd_base = s_off[tp - 1] + (int64_t)s_cnt[tp - 1];
    // ---- genotype rows -> LDS (coalesced along the row)
    stage_geno_rows<TPC>(g, s_snp, tp, tid, row_len, GS, s_g);
    // ---- phase 1
    if (tid < 64) {
      const bool on = ti1 < tp;
      const uint32_t cnt = on ? s_cnt[ti1] : 0u;
      const int64_t off = on ? s_off[ti1] : 0;
      const uint32_t rd4 = load_rd4(pv, off, cnt);       // the first four read bytes in one load (one dependent latency instead of four)
      double pG[9];
      const double mx = pair_values_open<9, 2, true>(pv, cnt, off, rd4, s_tab, wA, wR, n1, pG);
      if (on) {
        const double y = rcp_refined(mx);                                    // numerators >= 1e-6, mx in [1e-6, 1+1e-6]
        ok &= llks00_term(gp0, s_snp[ti1], [&](int l, int m) { const double v = div_by(pG[l * 3 + m], mx, y); s_pG[(ti1 * 2 + n1) * 9 + l * 3 + m] = v; return v; },
                    s_log, &s_t00[n1 * T00 + ti1]);                      // :656-663 into the llks00 term
      }
    }
    DMX_K2_SYNC();
    // ---- llks00: lane n < 2 of the cell adds its alpha's terms in pair order
    if (tid < 2) {
      const double* row = &s_t00[tid * T00];
      if (tp == TP) {                              // loads first (LDS latency paid once), then the ordered adds
        double2 v[TP / 2];
#pragma unroll
        for (int i = 0; i < TP / 2; ++i) v[i] = *reinterpret_cast<const double2*>(&row[2 * i]);
#pragma unroll
        for (int i = 0; i < TP / 2; ++i) { acc00 += v[i].x; acc00 += v[i].y; }
      } else {
        for (int i = 0; i < tp; ++i) acc00 += row[i];
      }
    }
    // ---- phase 2, in sub-tiles of SUB pairs.  FAST (bilinear) form: the nine-term sum g_j' pG[n] g_k is factored as
    // g_j . u with u[l] = sum_m pG[n][l][m] g_k[m] formed ONCE per (pair, alpha, k) and shared through LDS by the rows j — three
    // fused multiply-adds per evaluation instead of nine products and seventeen multiply/adds.  The value of a term moves by a
    // few ulp (<= ~1e-15 absolute); the accumulation order is the reference's, so the result stays within ~1e-11 of STRICT.
    if (!SHARE) {
      if (owner) {
        for (int ti = 0; ti < tp; ++ti) {
          const double* P = &s_pG[ti * 18];
          double P0[9], P1[9];
#pragma unroll
          for (int i = 0; i < 9; ++i) { P0[i] = P[i]; P1[i] = P[9 + i]; }
          const float* gr = &s_g[ti * GS];
          const double a0 = (double)gr[j * 3], a1 = (double)gr[j * 3 + 1], a2 = (double)gr[j * 3 + 2];
#pragma unroll
          for (int kk = 0; kk < NK; ++kk) {
            const int k = min(kb * NK + kk, V - 1);
            const double b0 = (double)gr[k * 3], b1 = (double)gr[k * 3 + 1], b2 = (double)gr[k * 3 + 2];
            double x[3], y[3];
#pragma unroll
            for (int l = 0; l < 3; ++l) {
              x[l] = __builtin_fma(P0[l * 3 + 2], b2, __builtin_fma(P0[l * 3 + 1], b1, P0[l * 3] * b0));
              y[l] = __builtin_fma(P1[l * 3 + 2], b2, __builtin_fma(P1[l * 3 + 1], b1, P1[l * 3] * b0));
            }
            const double s0 = __builtin_fma(a2, x[2], __builtin_fma(a1, x[1], a0 * x[0]));
            const double s1 = __builtin_fma(a2, y[2], __builtin_fma(a1, y[1], a0 * y[0]));
            ok &= __builtin_amdgcn_class(s0, 0x100) && __builtin_amdgcn_class(s1, 0x100);
            acc[kk][0] += dmx_log2_fastmode(s0, s_log, lk);
            acc[kk][1] += dmx_log2_fastmode(s1, s_log, lk);
          }
        }
      }
      DMX_K2_SYNC();
    } else
#pragma unroll 1
    for (int sub = 0; sub < tp; sub += SUB) {
      const int ns = min(SUB, tp - sub);
#pragma unroll 1
      for (int e = tid; e < ns * 2 * V; e += TPC) {
        const int k = e % V, n = (e / V) & 1, pi = e / (2 * V);
        const double* P = &s_pG[((sub + pi) * 2 + n) * 9];
        const float* gr = &s_g[(sub + pi) * GS + k * 3];
        const double b0 = (double)gr[0], b1 = (double)gr[1], b2 = (double)gr[2];
        double* u = &s_u[(size_t)((pi * 2 + n) * VU + k) * 4];
#pragma unroll
        for (int l = 0; l < 3; ++l) u[l] = __builtin_fma(P[l * 3 + 2], b2, __builtin_fma(P[l * 3 + 1], b1, P[l * 3] * b0));
      }
      DMX_K2_SYNC();
      if (owner) {
#pragma unroll 1
        for (int pi = 0; pi < ns; ++pi) {
          const float* gr = &s_g[(sub + pi) * GS];
          const double a0 = (double)gr[j * 3], a1 = (double)gr[j * 3 + 1], a2 = (double)gr[j * 3 + 2];
          const double* u0 = &s_u[(size_t)((pi * 2 + 0) * VU) * 4];
          const double* u1 = &s_u[(size_t)((pi * 2 + 1) * VU) * 4];
#pragma unroll
          for (int kk = 0; kk < NK; ++kk) {
            const int k = min(kb * NK + kk, V - 1);
            const double2 x01 = *reinterpret_cast<const double2*>(&u0[k * 4]);
            const double x2 = u0[k * 4 + 2];
            const double2 y01 = *reinterpret_cast<const double2*>(&u1[k * 4]);
            const double y2 = u1[k * 4 + 2];
            const double s0 = __builtin_fma(a2, x2, __builtin_fma(a1, x01.y, a0 * x01.x));
            const double s1 = __builtin_fma(a2, y2, __builtin_fma(a1, y01.y, a0 * y01.x));
            ok &= __builtin_amdgcn_class(s0, 0x100) && __builtin_amdgcn_class(s1, 0x100);
            acc[kk][0] += dmx_log2_fastmode(s0, s_log, lk);
            acc[kk][1] += dmx_log2_fastmode(s1, s_log, lk);
          }
        }
      }
      DMX_K2_SYNC();
    }
    DMX_K2_SYNC();
  }
  if (cell_ok) {
    if (owner) {
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        const int k = kb * NK + kk;
        if (k < V) {
          double* o = grid + (((size_t)cell * V + j) * V + k) * A;
          o[0] = acc[kk][0]; o[1] = acc[kk][1];
        }
      }
    }
    if (tid < 2 && blockIdx.y == 0) l00[(size_t)cell * A + tid] = acc00;
    if (!ok) flag_cell(flagged, cell);
  }
#undef DMX_K2_SYNC
}

// ---------------------------------------------------------------------------------------------------------------------
// K2, FAST mode, alpha grid {0, 0.5} (demuxlet's default): only the grid entries demuxlet ever prints or decides on.
//   * llksAB[j][k][0] for k != 0 is read by nothing but the maxLLK scan (cmd_cram_demuxlet.cpp:713-721; the printed uses of the
//     alpha[0] entries are [j][0][0] only, :726,:749-757,:774-780,:816-825), and maxLLK cancels in every printed posterior
//     (:726-733,:768,:780,:792,:827-828).  With alpha[0] == 0 the entry does not depend on k beyond float32 rounding of
//     sum_m g_k[m].  They are not computed; the grid cells are filled with [j][0][0].
//   * at alpha == 0.5 the mixture is symmetric: [k][j][1] is [j][k][1] up to the rounding of the nine-term sum (<= 3e-14 in the
//     reference), .pair prints j < k only (:785) and the host tie arbiter settles which order .best names.  One
//     evaluation per unordered pair {j,k}, mirrored into both cells.
// Per covered pair that is V + V(V+1)/2 log terms instead of 2 V^2: 560 instead of 2048 at V = 32.  Everything else follows
// k_doublet_a2f: the bilinear factoring g_j . u_k with u_k[l] = sum_m pG[1][l][m] g_k[m] formed once per (pair, k); every
// accumulator is owned by one lane which adds its terms in ascending SNP order (what keeps the result within ~1e-11 of STRICT).
// Entry e = tid + TPC*i of a lane: e < V*D (D = V/2 + 1): j = e % V, k = (j + e / V) % V at alpha 0.5 (the rotation makes the
// lanes of a wavefront read consecutive u_k: conflict-free LDS); V*D <= e < V*D + V: the singlet entry [j][0][0], j = e - V*D.
// For even V the offset d = V/2 is computed from both sides; only the j < k copy is stored.
// Panels wider than 64 samples cut the entry list into slabs of NEP entries per lane, one workgroup (blockIdx.y) per slab: each slab
// repeats the per-tile phases (cheap next to 256 * NEP evaluations per pair) and owns its entries' accumulators.
template <int TPC, int VMAX, int SUB, bool FIXJ, int MINW = 3, int NEP = 0, bool CHK = true>   // CHK: see k_doublet_a2
__global__ __launch_bounds__(kThreads, MINW) void k_doublet_sym(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                          const double* __restrict__ gp0, const double* __restrict__ tabs,
                                                          const int32_t* __restrict__ sched, int32_t V_and_flags,
                                                          double* __restrict__ grid, double* __restrict__ l00,
                                                          uint8_t* __restrict__ flagged, const double* __restrict__ pfin, const double* __restrict__ pseed) {
  // pfin (round 6; NULL: none): k_build_certify_finals' table — the finished phase-1 values of pairs of up to three tabled reads; pseed (NULL: none):
  // k_build_certify_seeds' table — the state after a pair's first one or two reads, for the pairs that walk the loop
  const int32_t V = V_and_flags & 0xFFFF;
  const bool no_dma = (V_and_flags >> 16) & 1;   // kernel experiments (DMX_SYM_NO_DMA; bit-identical results)
#if DMX_SYM_ABLATIONS                             // timing builds only (tools/build_variant.sh ... -DDMX_SYM_ABLATIONS=1): each switch drops one part of the
                                                  // kernel — results WRONG, time right.  The shipped library does not contain them.
  const bool abl_p1 = (V_and_flags >> 17) & 1;   // DMX_SYM_ABLATE_P1: phase 1's global loads all hit the same lines
  const bool abl_p2 = (V_and_flags >> 18) & 1;   // DMX_SYM_ABLATE_P2: no phase-2 evaluations
  const bool abl_u = (V_and_flags >> 19) & 1;    // DMX_SYM_ABLATE_U: u is not formed
  const bool abl_00 = (V_and_flags >> 21) & 1;   // DMX_SYM_ABLATE_00: no llks00 sums
#else
  constexpr bool abl_p1 = false, abl_p2 = false, abl_u = false, abl_00 = false;
#endif
  const bool no_prod = (V_and_flags >> 22) & 1;  // kernel experiment (DMX_SYM_NO_PRODUCT): a log per term also in full sub-tiles
  const bool no_pipe = (V_and_flags >> 23) & 1;  // kernel experiment (DMX_SYM_NO_PIPE; bit-identical results): phase 2 without the software pipeline
  const bool wait_all = (V_and_flags >> 24) & 1; // test switch (DMX_SYM_WAIT_ALL; bit-identical results): vmcnt(0) instead of the three-buffer form's counted wait
  // Narrow panels put SEVERAL barcodes in one wavefront (TPC = 32: two, TPC = 16: four): their entries fill the lanes (V = 16: 160
  // entries = 5 per lane of 32; V = 8: 48 = 3 per lane of 16) and the per-tile phases 0-1 are shared instruction-wise.  The tile is
  // what one pass of phase 1 covers: two lanes per pair.
  static_assert(TPC == 16 || TPC == 32 || TPC == 64 || TPC == 256, "threads per barcode");
  constexpr int A = 2, TP = TPC >= 64 ? 32 : TPC / 2;
  static_assert(SUB <= TP && TP % 8 == 0, "sub-tile");
  constexpr int CPW = kThreads / TPC;            // cells per workgroup
  constexpr int T00 = TP + 2;
  constexpr int NE = NEP ? NEP : (VMAX * (VMAX / 2 + 1) + VMAX + TPC - 1) / TPC;   // entries per lane (and slab)
  const int e_base = NEP ? (int)blockIdx.y * NEP * TPC : 0;         // first entry of this slab
  constexpr int VUS = (VMAX + 2) & ~1;           // u row stride (V alpha-0.5 rows + the alpha-0 row of sample 0), even
  constexpr int GSS = (3 * VMAX + 3) & ~3;       // genotype row stride (floats)
#define DMX_K2_SYNC() do { if (TPC <= 64) { DMX_WAVE_LDS_ORDER(); } else { __syncthreads(); } } while (0)
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_tab[kTab2];
  __shared__ double s_w[2][10];                  // mixing weights of :613 per alpha and distinct value: [n][0..4] = p (ALT), [n][5..9] = 1 - p
  __shared__ __attribute__((aligned(256))) double s_log32[DMX_LOG32_TABLE_DOUBLES];   // dmx_log2_lite32's rc[32] | logc[32]
  const double* s_log = s_tab + kLut2;
  const int t = threadIdx.x;
  stage_k2_tables(s_tab, tabs, t, kThreads);
  if (t < DMX_LOG32_TABLE_DOUBLES) s_log32[t] = tabs[kTabLog32 + t];
  // Round 6: WHICH of the two FAST logs an entry takes is a compile-time function of its slot i in the lane's entry list (so every accumulator sees one log
  // for the whole run, in every code path of this instantiation): dmx_log2_lite (256 bins, 16-byte gather with bank conflicts, 6 FP64 instructions) loads the
  // LDS, dmx_log2_lite32 (split 32-bin table, conflict-free, 8) loads the VALU — mixing them balances the two units that bind this kernel.
  constexpr int HYB = (FIXJ && MINW == 3 && NEP == 0 && DMX_FAST_LITE_LOG) ? DMX_SYM_HYB : 0;
  auto kind32 = [](int i) constexpr { return HYB == 3 || (HYB == 1 && i % 3 == 2) || (HYB == 2 && i % 3 != 0) || (HYB == 4 && (i & 1)); };
  const DmxLog32Pins lk32 = dmx_log32_pins();
  if (t < 10) {
    // alpha 0: p = 0.5 l does not depend on m -> slots 0..2 hold l = 0..2 (slots 3, 4 repeat l = 2); alpha 0.5: p = 0.25 (l + m)
    // -> slot = l + m.  Same operands, same operations as the nine entries of the reference: the values are bit-identical.
    const int n = t / 5, q = t % 5;
    const int l = n ? (q > 2 ? 2 : q) : min(q, 2), m = n ? q - l : 0;
    const double p = 0.5 * l + (m - l) * 0.5 * (n ? 0.5 : 0.0);
    s_w[n][q] = p;
    s_w[n][5 + q] = 1.0 - p;
  }
  __syncthreads();

  const int cw = t / TPC, tid = t % TPC;         // cell slot inside the workgroup, thread inside the cell
  // Up to two barcodes per wavefront (TPC >= 32): the genotype rows of a sub-tile go from global memory
  // straight into the LDS (global_load_lds: no registers, uniform source base per row), one sub-tile ahead of their use, into the
  // other half of a double buffer — the first sub-tile's while phase 1 runs.  cfg3 FAST: 394 -> 349 ms on one box.
  constexpr bool DMA_T = TPC >= 32;              // (four barcodes per wavefront, TPC = 16: too many small masked loads, measured +17 %)
  // row buffers: two (the next sub-tile's rows travel while this one computes) — THREE for the two-barcodes-per-wavefront form (V <= 16, small rows:
  // round 5), whose sparse workloads gather rows from a matrix beyond the L2 (cfg5: 38 MB) and waited for them half of their time with one sub-tile of lead
  constexpr int NBUF = DMA_T ? (TPC == 32 ? 3 : 2) : 1;
  constexpr size_t cell_bytes = (size_t)TP * 6 * 8 + (size_t)TP * 4 * 8 + 2 * T00 * 8 + TP * (4 + 4 + 8) + (size_t)NBUF * SUB * GSS * 4 + (size_t)SUB * 3 * VUS * 8;
  unsigned char* base = s_raw + (size_t)cw * cell_bytes;
  double* s_q1 = (double*)base;                                  // [TP][6]    pG of alpha 0.5: q[l+m], five distinct values
  double* s_u0 = s_q1 + TP * 6;                                  // [TP][4]    u of (alpha 0, sample 0)
  double* s_t00 = s_u0 + TP * 4;                                 // [2][T00]   llks00 terms
  int64_t* s_off = (int64_t*)(s_t00 + 2 * T00);                  // [TP]
  int32_t* s_snp = (int32_t*)(s_off + TP);                       // [TP]
  uint32_t* s_cnt = (uint32_t*)(s_snp + TP);                     // [TP]
  float* s_g0 = (float*)(s_cnt + TP);                            // [SUB][GSS] genotype rows of the sub-tile's SNPs (DMA: x 2)
  double* s_u = (double*)(s_g0 + NBUF * SUB * GSS);              // [SUB][3][VUS]

  const int slot = blockIdx.x * CPW + cw;
  if (TPC == 64 && slot >= pv.B) return;         // whole wavefront idle (no workgroup barriers below in this mode)
  const bool cell_ok = slot < pv.B;              // (sub-wavefront barcodes past the end stay in the wavefront with zero pairs)
  const int32_t cell = cell_ok ? sched[slot] : 0;
  const int64_t p_beg = cell_ok ? pv.cell_pair_off[cell] : 0;
  const int64_t np = cell_ok ? pv.cell_pair_off[cell + 1] - p_beg : 0;
  int64_t rd_base = cell_ok ? pv.cell_read_off[cell] : 0;

  // phase-2 identity: NE entries per lane
  const int D = V / 2 + 1, VD = V * D;
  int ek[NE], ej[NE];                            // u row (k, or V = the alpha-0 row) and sample j of each entry
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int e = e_base + tid + TPC * i;
    if (e < VD) { const int j = e % V; int k = j + e / V; k = k >= V ? k - V : k; ej[i] = j; ek[i] = k; }
    else if (e < VD + V) { ej[i] = e - VD; ek[i] = V; }
    else { ej[i] = 0; ek[i] = V; }               // idle slot: computes the first singlet term, never stored
  }
  double acc[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) acc[i] = 0.0;
  // u-formation identity: entry tid + TPC * i of a sub-tile's SUB * V (pair, sample) values
  constexpr int NU = (SUB * VMAX + TPC - 1) / TPC;
  int uq[NU];                                    // (pair << 16) | sample; negative: no such entry
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const int e = tid + TPC * i;
    uq[i] = e < SUB * V ? ((e / V) << 16) | (e % V) : (int)0x80000000;
  }
  bool ok = true;
  const DmxLogPins lk = dmx_log_pins();
  // phase-1 identity (first wavefront of the cell): pair ti1, alpha n1
  const int ti1 = tid >> 1, n1 = tid & 1;
  double acc00 = 0.0;                            // lane n1 == tid < 2 owns llks00[n]
  const int row_len = V * 3;

  // Narrow panels (short tiles, several barcodes per wavefront) request a tile's header one tile ahead; the wide forms have no
  // register to spare for it (9 entries per lane at 167 VGPRs) and hide that latency behind their longer phase 2.
  constexpr bool PREFETCH = TPC < 64;
  uint32_t hd_n = 0u; int32_t hd_s = 0;          // header (stored reads, SNP id) of this lane's pair in the NEXT tile
  if (PREFETCH && tid < TP && tid < np) { hd_n = load_nrd(pv.pair_nrd, p_beg + tid, nrd_width); hd_s = pv.pair_snp ? pv.pair_snp[p_beg + tid] : (int32_t)tid; }
  const bool dma = DMA_T && !no_dma;
  auto request_rows = [&](int sub, int buf) {    // rows of the pairs sub .. sub+SUB-1 of the current tile -> s_g0[buf], asynchronously
    using gptr = const __attribute__((address_space(1))) void*;
    using lptr = __attribute__((address_space(3))) void*;
    const int wv = tid & ~63;                      // first lane of this wavefront inside the cell
    constexpr int SPW = TPC >= 64 ? 1 : 64 / TPC;
    const int slot = SPW == 1 ? 0 : (threadIdx.x & 63) / TPC;
    // (a ROLLED loop over the slots: with the slots as separate branches the compiler merges their identical tails into one
    //  instruction that serves lanes of two barcodes with one LDS base — it takes the base operand for uniform)
#pragma unroll 1
    for (int c = 0; c < SPW; ++c) {
      if (SPW == 1 || slot == c) {
#pragma unroll
    for (int pi = 0; pi < SUB; ++pi) {             // a row at a time: uniform source base, lane r reads element r
      const float* src = g + (size_t)__builtin_amdgcn_readfirstlane(s_snp[sub + pi]) * row_len;
#pragma unroll
      for (int h = 0; h < (GSS + TPC - 1) / TPC; ++h) {
        const int r = tid + TPC * h;
        // (a piece with no element of the row is skipped by the whole barcode: TPC * h < row_len is uniform, so the number of loads a request
        //  puts in flight is SUB * ceil(row_len / TPC) exactly — what the counted wait of the three-buffer form relies on)
        if (TPC * h < row_len && r < row_len) __builtin_amdgcn_global_load_lds((gptr)(src + r), (lptr)(s_g0 + (buf * SUB + pi) * GSS + wv + TPC * h - c * TPC), 4, 0, 0);
      }
    }
      }
    }
  };
  for (int64_t tbase = 0; tbase < np; tbase += TP) {
    const int tp = (int)min((int64_t)TP, np - tbase);
    // ---- headers of the tile's pairs (first 32 lanes of the cell)
    if (tid < TP) {
      uint32_t n; int32_t sn;
      if (PREFETCH) {                              // this tile's header was requested a tile ago; now request the next one's
        n = hd_n; sn = hd_s;
        const int64_t nx = tbase + TP + tid;
        hd_n = 0u; hd_s = 0;
        if (nx < np) { hd_n = load_nrd(pv.pair_nrd, p_beg + nx, nrd_width); hd_s = pv.pair_snp ? pv.pair_snp[p_beg + nx] : (int32_t)nx; }
      } else {
        const bool v = tid < tp;
        n = v ? load_nrd(pv.pair_nrd, p_beg + tbase + tid, nrd_width) : 0u;
        sn = v ? (pv.pair_snp ? pv.pair_snp[p_beg + tbase + tid] : (int32_t)(tbase + tid)) : 0;
      }
      publish_tile_headers<TP>(n, sn, tid, rd_base, s_cnt, s_off, s_snp);
    }
    DMX_K2_SYNC();
    rd_base = s_off[tp - 1] + (int64_t)s_cnt[tp - 1];
    if (dma) {
      request_rows(0, 0);                          // sub-tile 0's rows travel while phase 1 runs
      if (NBUF == 3 && SUB < tp) request_rows(SUB, 1);
    }
    // ---- phase 1: pG[n][3][3] of the pair (:600-663), exactly as k_doublet_a2; kept: alpha 0.5's nine values, and for
    //      alpha 0 the three u values of sample 0 (the only k the singlet column [j][0][0] needs)
    if (tid < 2 * TP) {
      const bool on = ti1 < tp;
      const uint32_t cnt = on ? s_cnt[ti1] : 0u;
      const int64_t off = on ? s_off[ti1] : 0;
      const uint32_t rd4 = load_rd4(pv, abl_p1 ? (off & 63) : off, cnt);       // the first four read bytes in one load (one dependent latency instead of four)
      const int32_t snp1 = on ? (abl_p1 ? (s_snp[ti1] & 15) : s_snp[ti1]) : 0;
      const float* g0r = g + (size_t)snp1 * row_len;             // sample 0's row (alpha-0 lanes use it)
      const float gf0 = g0r[0], gf1 = g0r[1], gf2 = g0r[2];
      double q[5];
      // Round 6: a pair of up to three tabled reads takes its FINISHED values from the table (one 64-byte entry per read code: the alpha = 0.5 lane its
      // five, the alpha = 0 lane its three); the read loop and the +1e-6 renormalisation below run only in tiles with a deeper pair (wave-uniform branch).
      // Timing builds: the loop is 22 of cfg3 FAST's 201 ms (a dependent chain — products, maximum, the neighbour's, reciprocal, quotients — per read,
      // with LDS look-ups in it), at 1.25 reads per pair 93 % of the tiles skip it.  Same operations on the same operands (k_build_certify_finals): same bits.
      // (a tile with a deeper pair runs the loop for ALL its lanes, as before: no merge of the two sources, no register held across the loop)
      const int32_t fi = pfin ? certify_final_index(cnt, rd4) : -1;
      if (!__any(fi < 0)) {
        const double* fp = pfin + (size_t)fi * kCFinStride + (n1 ? 0 : 5);
        q[0] = fp[0]; q[1] = fp[1]; q[2] = fp[2];
        q[3] = n1 ? fp[3] : 0.0; q[4] = n1 ? fp[4] : 0.0;
      } else {
        // the loop of :597-639 and the +1e-6 renormalisation (:649-663) — k_certify's function (each lane keeps its own alpha's values): on the default
        // grid a pair's first one or two reads come from the seed table (round 6 for this kernel: the loop starts at read 1 or 2 — what matters for pileups
        // too deep for the final-value table, cfg5's 2 reads per pair)
        double wA[5], wR[5];                                               // the weights live in registers during phase 1 only
#pragma unroll
        for (int i = 0; i < 5; ++i) { wA[i] = s_w[n1][i]; wR[i] = s_w[n1][5 + i]; }
        certify_pair_values<5, false>(pv, cnt, off, rd4, s_tab, wA, wR, n1, q, pseed);
      }
      if (on) {
        const double* g0 = gp0 + (size_t)snp1 * 3;
        const double q0 = g0[0], q1 = g0[1], q2 = g0[2];
        const double qq[3] = {q0, q1, q2};
        double sum = 0.0;
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            const double v = n1 ? q[l + m] : q[l];                           // pG[n][l][m] (not llks00_term: the call selects q[] with fewer instructions, another kernel)
            sum += ((qq[l] * qq[m]) * v);                                    // gp00 (:555) then :702-705
          }
        ok &= __builtin_amdgcn_class(sum, 0x100);
        s_t00[n1 * T00 + ti1] = dmx_log2_fast(sum, s_log);                    // :708-709 term
        if (n1) {
#pragma unroll
          for (int i = 0; i < 5; ++i) s_q1[ti1 * 6 + i] = q[i];
        } else {
          const double b0 = (double)gf0, b1 = (double)gf1, b2 = (double)gf2;
#pragma unroll
          for (int l = 0; l < 3; ++l) s_u0[ti1 * 4 + l] = __builtin_fma(q[l], b2, __builtin_fma(q[l], b1, q[l] * b0));
        }
      }
    }
    DMX_K2_SYNC();
    // ---- llks00: lane n < 2 of the cell adds its alpha's terms in pair order
    if (tid < 2 && !abl_00) {
      const double* row = &s_t00[tid * T00];
      if (tp == TP) {                              // eight terms at a time: loads first, then the ordered adds
#pragma unroll 1
        for (int h = 0; h < TP; h += 8) {
          double2 v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const double2*>(&row[h + 2 * i]);
#pragma unroll
          for (int i = 0; i < 4; ++i) { acc00 += v[i].x; acc00 += v[i].y; }
        }
      } else {
        for (int i = 0; i < tp; ++i) acc00 += row[i];
      }
    }
    // ---- phase 2 in sub-tiles of SUB pairs
#pragma unroll 1
    for (int sub = 0; sub < tp; sub += SUB) {
      const int ns = min(SUB, tp - sub);
      const int buf = dma ? (NBUF == 3 ? (sub / SUB) % 3 : (sub / SUB) & 1) : 0;
      float* s_g = s_g0 + buf * SUB * GSS;
      if (dma) {
        if constexpr (NBUF == 3) {
          // this sub-tile's rows have landed when at most the loads THIS BARCODE requested after them are in flight (loads return in order): kReq = SUB
          // rows x pieces per row, per request and barcode (request_rows).  The wavefront's other barcode issues its own requests in between (or
          // none: its tile may be shorter), which can only make this wait longer, never too short.
          static_assert((GSS + TPC - 1) / TPC <= 2 && 2 * SUB <= 15, "vmcnt field / pieces per row");
          // (the count is safe only while request_rows issues EXACTLY SUB x pieces loads per barcode — its `TPC * h < row_len` test is uniform and its
          //  slot loop rolled for that reason; tests/test_gpu_parity.py::test_counted_row_wait_equals_waiting_for_everything compares this form with
          //  wait_all bit for bit on partial last sub-tiles, barcodes of unequal length in one wavefront and every V the form serves)
          if (sub + SUB >= tp || wait_all) __builtin_amdgcn_s_waitcnt(0x0F70);                // nothing requested after them: vmcnt(0)
          else if (row_len > TPC) __builtin_amdgcn_s_waitcnt(0x0F70 | (2 * SUB));             // vmcnt(kReq), two pieces per row
          else __builtin_amdgcn_s_waitcnt(0x0F70 | SUB);                                      // one piece per row
          if (sub + 2 * SUB < tp) request_rows(sub + 2 * SUB, (buf + 2) % 3);   // two sub-tiles ahead (that buffer was last read a sub-tile ago, two syncs back)
        } else {
          __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): this sub-tile's rows have landed ...
          if (sub + SUB < tp) request_rows(sub + SUB, buf ^ 1);   // ... the next one's take off (its buffer was last read two syncs ago)
        }
      } else {
      // genotype rows of the sub-tile -> LDS (coalesced along the row)
        int r = tid % row_len, pi = tid / row_len;
        const int dr = TPC % row_len, dt = TPC / row_len;
        while (pi < ns) {
          s_g[pi * GSS + r] = g[(size_t)s_snp[sub + pi] * row_len + r];
          r += dr; pi += dt;
          if (r >= row_len) { r -= row_len; ++pi; }
        }
      }
      DMX_K2_SYNC();
      // u[pi][l][k] = sum_m pG[1][l][m] g_k[m]  (k < V), and row V = the alpha-0 u of sample 0.  Round 5: the lane's NU entries are formed TOGETHER,
      // branch-free, with the (pair, k) of each entry computed once per kernel — as a rolled loop with a division and a branch per entry this step
      // was a fifth of the kernel (timing builds without it: cfg3 FAST 95 -> 49 ms of 247, cfg5 FAST 29.9 -> 20.4 of 45.8), three exposed LDS round
      // trips per entry for 9 multiply-adds.
      if (!abl_u) {
        if (tid < ns * 3) { const int pi = tid / 3, l = tid - 3 * pi; s_u[(size_t)pi * 3 * VUS + l * VUS + V] = s_u0[(sub + pi) * 4 + l]; }
        double un[NU][3];
#pragma unroll
        for (int i = 0; i < NU; ++i) {
          const int pi = (uq[i] >> 16) & 0x7FFF, k = uq[i] & 0xFFFF;        // (an entry past the sub-tile's SUB * V: pair 0, sample 0, not stored)
          const double* P = &s_q1[(sub + pi) * 6];                 // pG[1][l][m] = P[l + m]
          const float* gr = &s_g[pi * GSS + k * 3];
          const double b0 = (double)gr[0], b1 = (double)gr[1], b2 = (double)gr[2];
#pragma unroll
          for (int l = 0; l < 3; ++l) un[i][l] = __builtin_fma(P[l + 2], b2, __builtin_fma(P[l + 1], b1, P[l] * b0));
        }
#pragma unroll
        for (int i = 0; i < NU; ++i) {
          const int pi = (uq[i] >> 16) & 0x7FFF, k = uq[i] & 0xFFFF;
          if (uq[i] >= 0 && pi < ns) {
            double* u = &s_u[(size_t)pi * 3 * VUS + k];
            u[0] = un[i][0]; u[VUS] = un[i][1]; u[2 * VUS] = un[i][2];
          }
        }
      }
      DMX_K2_SYNC();
      constexpr int UPI = MINW >= 4 ? 1 : SUB;       // pairs unrolled together (register budget)
      // Round-5 experiment (DMX_FAST_PRODUCT builds only; not shipped): a full sub-tile takes ONE log per entry — of the product of its SUB terms
      // (a multiply per term; the log's ~13 instructions and its table read once per SUB terms).  Every term is in [1e-66, 1e78] when k_check_geno
      // has passed the rows, and realistic ones in [1e-6, 1]: a product of four is a normal number, and the result is CLOSER to the exact sum than
      // the reference's.  That is the problem: the reference's llk carries the rounding of its own 50 000 adds (half an ulp of the running sum each,
      // rms 2e-12 at cfg3's depth), which only the same adds of the same terms reproduce — the per-term form agrees with it to 4e-11, this one to 1.3e-9.
      constexpr bool PROD = !CHK && SUB <= 4 && DMX_FAST_PRODUCT;
      constexpr int NB = DMX_SYM_NB > 0 ? DMX_SYM_NB : 1;
      constexpr bool PIPE2 = FIXJ && DMX_SYM_NB > 0 && DMX_FAST_LITE_LOG && !PROD && MINW == 3 && NEP == 0;
      if (PROD && ns == SUB && !abl_p2 && !no_prod) {
        double a[SUB][3];
        if (FIXJ) {
#pragma unroll
          for (int pi = 0; pi < SUB; ++pi) {
            const float* gr = &s_g[pi * GSS + ej[0] * 3];
            a[pi][0] = (double)gr[0]; a[pi][1] = (double)gr[1]; a[pi][2] = (double)gr[2];
          }
        }
#pragma unroll
        for (int i = 0; i < NE; ++i) {
          double pr = 1.0;
#pragma unroll
          for (int pi = 0; pi < SUB; ++pi) {
            if (!FIXJ) {
              const float* gr = &s_g[pi * GSS + ej[i] * 3];
              a[pi][0] = (double)gr[0]; a[pi][1] = (double)gr[1]; a[pi][2] = (double)gr[2];
            }
            const double* up = &s_u[pi * 3 * VUS];
            const double x0 = DMX_LDS_NOMERGE ? lds_read_f64(&up[ek[i]]) : up[ek[i]], x1 = DMX_LDS_NOMERGE ? lds_read_f64(&up[VUS + ek[i]]) : up[VUS + ek[i]],
                         x2 = DMX_LDS_NOMERGE ? lds_read_f64(&up[2 * VUS + ek[i]]) : up[2 * VUS + ek[i]];
            const double sj = __builtin_fma(a[pi][2], x2, __builtin_fma(a[pi][1], x1, a[pi][0] * x0));
            pr = pi ? pr * sj : sj;
          }
          acc[i] += dmx_log2_fastmode(pr, s_log, lk);
        }
      } else if (PIPE2 && ns == SUB && !abl_p2 && !no_pipe) {
        // Round 6: a full sub-tile's SUB x NE evaluations as ONE software-pipelined sequence of steps of NB entries (pair-major, so that every
        // accumulator still adds its terms in ascending pair order: the same operations on the same operands as the loop below — same bits).
        // Left to the compiler, a pair's entries were evaluated two at a time with three EXPOSED LDS round trips per two evaluations (u, then each
        // log's table entry) and only three wavefronts per SIMD to hide them behind: the kernel issued on half of its cycles.  Here step s + 1's
        // u values are requested, and step s's table entries, BEFORE the polynomial and the add of step s - 1 run: no wait in the steady state.
        constexpr int NBAT = (NE + NB - 1) / NB, NST = SUB * NBAT;
        double xu[NB][3];                            // u values of the step whose dot products come next
        double zq[2][NB]; int32_t kq[2][NB]; double2 tq[2][NB];   // per step: reduced argument, binary exponent << 20, table entry {1/c, log c}
        double a0, a1, a2;
        auto load_u = [&](int st) {
          const int pi = st / NBAT, b0 = (st % NBAT) * NB;
          const double* up = &s_u[pi * 3 * VUS];
#pragma unroll
          for (int q = 0; q < NB; ++q) if (b0 + q < NE) {
            xu[q][0] = lds_read_f64(&up[ek[b0 + q]]); xu[q][1] = lds_read_f64(&up[VUS + ek[b0 + q]]); xu[q][2] = lds_read_f64(&up[2 * VUS + ek[b0 + q]]);
          }
        };
        auto load_a = [&](int pi) { const float* gr = &s_g[pi * GSS + ej[0] * 3]; a0 = (double)gr[0]; a1 = (double)gr[1]; a2 = (double)gr[2]; };
        load_a(0);
        load_u(0);
#pragma unroll
        for (int st = 0; st <= NST; ++st) {
          const int cur = st & 1, prv = cur ^ 1;
          if (st < NST) {
            const int b0 = (st % NBAT) * NB;
#pragma unroll
            for (int q = 0; q < NB; ++q) if (b0 + q < NE) {         // dot product, argument reduction, table request (dmx_log2_lite, first half)
              const double sj = __builtin_fma(a2, xu[q][2], __builtin_fma(a1, xu[q][1], a0 * xu[q][0]));
              if (CHK) ok &= __builtin_amdgcn_class(sj, 0x100);
              const uint32_t hi = (uint32_t)__double2hiint(sj), lo = (uint32_t)__double2loint(sj);
              const uint32_t tmp = hi - (kind32(b0 + q) ? DMX_LOG32_OFF_HI : DMX_LOG2_OFF_HI);
              const uint32_t k20 = tmp & 0xFFF00000u;
              zq[cur][q] = __hiloint2double((int)(hi - k20), (int)lo);
              kq[cur][q] = (int32_t)k20;
              if (kind32(b0 + q)) {
                const char* e32 = reinterpret_cast<const char*>(s_log32) + ((tmp >> 12) & 0xF8u);
                tq[cur][q].x = lds_read_f64(reinterpret_cast<const double*>(e32));
                tq[cur][q].y = lds_read_f64(reinterpret_cast<const double*>(e32 + 256));
              } else
              tq[cur][q] = *reinterpret_cast<const double2*>(reinterpret_cast<const char*>(s_log) + ((tmp >> 8) & 0xFF0u));
            }
            if (st + 1 < NST) {
              if ((st + 1) % NBAT == 0) load_a((st + 1) / NBAT);
              load_u(st + 1);
            }
            __builtin_amdgcn_sched_barrier(0);                       // requests first: nothing of the arithmetic below moves above them
          }
          if (st > 0) {
            const int b0 = ((st - 1) % NBAT) * NB;
#pragma unroll
            for (int q = 0; q < NB; ++q) if (b0 + q < NE) {         // dmx_log2_lite, second half, and the ordered add
              const double r = __builtin_fma(zq[prv][q], tq[prv][q].x, -1.0);
#if DMX_SYM_TIMING & 2
              const double w = tq[prv][q].y + lds_read_f64(reinterpret_cast<const double*>(reinterpret_cast<const char*>(s_log) + 1024 + (kq[prv][q] >> 17)));
#else
              const double kd = (double)kq[prv][q];
              const double w = __builtin_fma(kd, 0x1.62e42fefa39efp-1 * 0x1p-20, tq[prv][q].y);
#endif
              double qq;
              if (kind32(b0 + q)) {
                qq = __builtin_fma(r, lk32.a5, lk32.a4);
                qq = __builtin_fma(r, qq, lk32.a3);
                qq = __builtin_fma(r, qq, lk32.a2);
              } else
              qq = __builtin_fma(r, lk.m14, lk.c13);
#if !(DMX_SYM_TIMING & 1)
              qq = __builtin_fma(r, qq, -0.5);
#endif
              qq = __builtin_fma(r, qq, 1.0);
              acc[b0 + q] += __builtin_fma(r, qq, w);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      } else
#pragma unroll UPI
      for (int pi = 0; pi < SUB; ++pi) {
        if (pi < ns && !abl_p2) {
          const float* gr = &s_g[pi * GSS];
          const double* up = &s_u[pi * 3 * VUS];
          double a0 = 0.0, a1 = 0.0, a2 = 0.0;
          if (FIXJ) { a0 = (double)gr[ej[0] * 3]; a1 = (double)gr[ej[0] * 3 + 1]; a2 = (double)gr[ej[0] * 3 + 2]; }
#pragma unroll
          for (int i = 0; i < NE; ++i) {
            if (!FIXJ) { a0 = (double)gr[ej[i] * 3]; a1 = (double)gr[ej[i] * 3 + 1]; a2 = (double)gr[ej[i] * 3 + 2]; }
            const double x0 = DMX_LDS_NOMERGE ? lds_read_f64(&up[ek[i]]) : up[ek[i]], x1 = DMX_LDS_NOMERGE ? lds_read_f64(&up[VUS + ek[i]]) : up[VUS + ek[i]],
                         x2 = DMX_LDS_NOMERGE ? lds_read_f64(&up[2 * VUS + ek[i]]) : up[2 * VUS + ek[i]];
            const double sj = __builtin_fma(a2, x2, __builtin_fma(a1, x1, a0 * x0));
            if (CHK) ok &= __builtin_amdgcn_class(sj, 0x100);
            acc[i] += kind32(i) ? dmx_log2_lite32(sj, s_log32, lk32) : dmx_log2_fastmode(sj, s_log, lk);
          }
        }
      }
      DMX_K2_SYNC();
    }
  }
  if (cell_ok) {
    double* G = grid + (size_t)cell * V * V * A;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = e_base + tid + TPC * i;
      if (e < VD) {
        const int j = ej[i], k = ek[i], d = e / V;
        if (!(2 * d == V && j > k)) {              // d = V/2 is reached from both sides: the j < k lane stores
          G[((size_t)j * V + k) * A + 1] = acc[i];
          G[((size_t)k * V + j) * A + 1] = acc[i];
        }
      } else if (e < VD + V) {
        const int j = ej[i];
        for (int k = 0; k < V; ++k) G[((size_t)j * V + k) * A] = acc[i];
      }
    }
    if (tid < 2 && e_base == 0) l00[(size_t)cell * A + tid] = acc00;
    if (!ok) flag_cell(flagged, cell);
  }
#undef DMX_K2_SYNC
}

// ---------------------------------------------------------------------------------------------------------------------
// K2 STRICT, default grid {0, 0.5}, 32 soft-field samples (cfg3 — the headline): k_doublet_a2's arithmetic with SYMMETRIC ownership (round 6).
// At alpha = 0.5 the mixture is symmetric, pG[1][l][m] == pG[1][m][l] bit for bit (equal mixing weights go through identical operations), so the nine
// terms (g_k[l] g_j[m]) pG[1][l][m] of entry [k][j] are the nine terms T[l][m] = (g_j[l] g_k[m]) pG[1][l][m] of entry [j][k], transposed: the reference adds
// them row-major for [j][k] and column-major for [k][j] — two different roundings of one set of products.  A lane that owns BOTH entries forms the exact
// products E[l][m] = g_j[l] g_k[m] once (they serve both entries at both alphas) and T once: 36 multiplies per unordered pair instead of 54, the 32 adds,
// four logs and four accumulator adds unchanged — 112 FP64 instructions where k_doublet_a2 spends 130, every operation the reference's on its operands
// in its order: the same bits (tests/test_gpu_parity.py::test_symmetric_strict_kernel_gives_k_doublet_a2s_bits).
// Ownership: lane (j = lane & 31, h = lane >> 5) of slab s (blockIdx.y, two per barcode) owns the unordered pairs {j, (j + d) & 31}, d = 1 + 2 (4 s + i) + h,
// i = 0..3 — d = 1..16, d = 16 from j < 16 only — with four accumulators each ([j][k][0], [j][k][1], [k][j][0], [k][j][1]), and slab 0 owns the diagonal:
// lane (j, h) the entry [j][j][h].  496 pairs x 112 + 64 x 37 instructions per covered pair against 1 024 x 65.  One wavefront per (barcode, slab), no
// workgroup barrier: each slab runs the cheap per-tile phases for itself (k_doublet_sym's: headers, rows straight into the LDS one sub-tile ahead, phase 1
// with the final-value table), then its pairs.
template <int SUB, int MINW, int NUP = 4>     // NUP = 0: the diagonal entries only (behind k_doublet_a2u, which owns everything else and llks00)
__global__ __launch_bounds__(kThreads, MINW) void k_doublet_a2s(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                          const double* __restrict__ gp0, const double* __restrict__ tabs,
                                                          const int32_t* __restrict__ sched,
                                                          double* __restrict__ grid, double* __restrict__ l00, const double* __restrict__ pfin) {
  constexpr int V = 32, A = 2, TP = 32, TPC = 64, CPW = kThreads / TPC, T00 = TP + 2, NU = NUP ? NUP : 1, GSS = 3 * V, row_len = 3 * V;
  constexpr bool DIAG_ONLY = NUP == 0;
  __shared__ double s_tab[kTab2];
  __shared__ double s_w[2][10];
  __shared__ __attribute__((aligned(16))) double s_pq_all[CPW][TP][8];       // per pair: alpha 0.5's five distinct values q[l + m] | alpha 0's three q[l]
  __shared__ double s_t00_all[CPW][2][T00];
  __shared__ int64_t s_off_all[CPW][TP];
  __shared__ int32_t s_snp_all[CPW][TP];
  __shared__ uint32_t s_cnt_all[CPW][TP];
  __shared__ __attribute__((aligned(16))) float s_g_all[CPW][2][SUB][GSS];
  const double* s_log = s_tab + kLut2;
  const int t = threadIdx.x;
  stage_k2_tables(s_tab, tabs, t, kThreads);
  if (t < 10) {                                  // the FIVE-form weights (k_doublet_sym): alpha 0: p = 0.5 l (slots 3, 4 repeat l = 2); alpha 0.5: p = 0.25 (l + m), slot l + m
    const int n = t / 5, q = t % 5;
    const int l = n ? (q > 2 ? 2 : q) : min(q, 2), m = n ? q - l : 0;
    const double p = 0.5 * l + (m - l) * 0.5 * (n ? 0.5 : 0.0);
    s_w[n][q] = p;
    s_w[n][5 + q] = 1.0 - p;
  }
  __syncthreads();
  const int cw = t / TPC, tid = t % TPC;
  double* s_pq = &s_pq_all[cw][0][0]; double* s_t00 = &s_t00_all[cw][0][0];
  int64_t* s_off = s_off_all[cw]; int32_t* s_snp = s_snp_all[cw]; uint32_t* s_cnt = s_cnt_all[cw];
  float* s_g0 = &s_g_all[cw][0][0][0];
  const int slot = blockIdx.x * CPW + cw;
  if (slot >= pv.B) return;                      // (no workgroup barrier below)
  const int slab = (int)blockIdx.y;
  const int32_t cell = sched[slot];
  const int64_t p_beg = pv.cell_pair_off[cell];
  const int64_t np = pv.cell_pair_off[cell + 1] - p_beg;
  int64_t rd_base = pv.cell_read_off[cell];
  const int j = tid & 31, h = tid >> 5;
  int kk[NU];
#pragma unroll
  for (int i = 0; i < NU; ++i) kk[i] = (j + 1 + 2 * (NU * slab + i) + h) & 31;
  double acc[NU][4];
#pragma unroll
  for (int i = 0; i < NU; ++i) { acc[i][0] = 0.0; acc[i][1] = 0.0; acc[i][2] = 0.0; acc[i][3] = 0.0; }
  double accd = 0.0, acc00 = 0.0;
  const DmxLogPins lk = dmx_log_pins();
  const int ti1 = tid >> 1, n1 = tid & 1;
  // the diagonal lane's value of (l, m): alpha 0.5 (h = 1) q[l + m] = s_pq[l + m], alpha 0 (h = 0) q[l] = s_pq[5 + l]: index (5 + l) + h (m - 5)
  const int dg[3] = {h * -5, h * -4, h * -3};
  auto request_rows = [&](int sub, int buf) {    // rows of the pairs sub .. sub+SUB-1 of the current tile -> s_g0[buf], asynchronously (k_doublet_sym)
    using gptr = const __attribute__((address_space(1))) void*;
    using lptr = __attribute__((address_space(3))) void*;
#pragma unroll
    for (int pi = 0; pi < SUB; ++pi) {
      const float* src = g + (size_t)__builtin_amdgcn_readfirstlane(s_snp[sub + pi]) * row_len;
#pragma unroll
      for (int hh = 0; hh < (GSS + TPC - 1) / TPC; ++hh) {
        const int r = tid + TPC * hh;
        if (r < row_len) __builtin_amdgcn_global_load_lds((gptr)(src + r), (lptr)(s_g0 + (buf * SUB + pi) * GSS + TPC * hh), 4, 0, 0);
      }
    }
  };
  for (int64_t tbase = 0; tbase < np; tbase += TP) {
    const int tp = (int)min((int64_t)TP, np - tbase);
    load_tile_headers<TP>(pv, nrd_width, p_beg, tbase, tp, tid, rd_base, s_cnt, s_off, s_snp);
    DMX_WAVE_LDS_ORDER();
    rd_base = s_off[tp - 1] + (int64_t)s_cnt[tp - 1];
    request_rows(0, 0);                            // sub-tile 0's rows travel while phase 1 runs
    // ---- phase 1 (:597-663): lane (pair ti1, alpha n1), five distinct values
    {
      const bool on = ti1 < tp;
      const uint32_t cnt = on ? s_cnt[ti1] : 0u;
      const int64_t off = on ? s_off[ti1] : 0;
      const uint32_t rd4 = load_rd4(pv, off, cnt);
      const int32_t snp1 = on ? s_snp[ti1] : 0;
      double q[5];
      const int32_t fi = pfin ? certify_final_index(cnt, rd4) : -1;
      if (!__any(fi < 0)) {
        const double* fp = pfin + (size_t)fi * kCFinStride + (n1 ? 0 : 5);
        q[0] = fp[0]; q[1] = fp[1]; q[2] = fp[2];
        q[3] = n1 ? fp[3] : 0.0; q[4] = n1 ? fp[4] : 0.0;
      } else {
        // (its own copy of certify_pair_values<5, false>: through the call k_doublet_a2s<4, 3, 4> spills 77 registers instead of 129: another kernel)
        double wA[5], wR[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) { q[i] = 1.0; wA[i] = s_w[n1][i]; wR[i] = s_w[n1][5 + i]; }   // :597
        for (uint32_t r = 0; __any(r < cnt); ++r) {
          const bool live = r < cnt;
          const uint32_t byte = live ? (r < 4 ? (rd4 >> (8 * r)) & 0xFFu : (uint32_t)pv.reads[off + r]) : 0u;
          const uint32_t bq = byte & 127u;
          const bool alt = (byte >> 7) != 0;
          const double pR = alt ? s_tab[128 + bq] : s_tab[bq];                // :606
          const double pA = alt ? s_tab[bq] : s_tab[128 + bq];                // :607
          double mx = 0.0;
          if (live) {
#pragma unroll
            for (int i = 0; i < 5; ++i) {
              q[i] *= (pR * wR[i] + pA * wA[i]);                              // :625
              mx = fmax(mx, q[i]);                                            // :626-627
            }
          }
          {
            const double o = shfl_xor1(mx);                                   // one max across both alphas of the pair
            mx = fmax(mx, o);
          }
          if (live) {
            if (cnt <= kSafeReads) {
              const double y = rcp_refined(mx);
#pragma unroll
              for (int i = 0; i < 5; ++i) q[i] = div_by(q[i], mx, y);         // :632-639
            } else {
#pragma unroll
              for (int i = 0; i < 5; ++i) q[i] = div_slow(q[i], mx);
            }
          }
        }
        double mx = 0.0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          q[i] += 1e-6;                                                        // :649
          mx = fmax(mx, q[i]);
        }
        {
          const double o = shfl_xor1(mx);
          mx = fmax(mx, o);
        }
        const double y = rcp_refined(mx);
#pragma unroll
        for (int i = 0; i < 5; ++i) q[i] = div_by(q[i], mx, y);                // :656-663
      }
      if (on) {
        const double* g0 = gp0 + (size_t)snp1 * 3;
        const double qq[3] = {g0[0], g0[1], g0[2]};
        double sum = 0.0;
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            const double v = n1 ? q[l + m] : q[l];                           // pG[n][l][m] (not llks00_term: the call selects q[] with fewer instructions, another kernel)
            sum += ((qq[l] * qq[m]) * v);                                    // gp00 (:555) then :702-705
          }
        s_t00[n1 * T00 + ti1] = dmx_log2_fast(sum, s_log);                    // :708-709 term
        if (n1) {
#pragma unroll
          for (int i = 0; i < 5; ++i) s_pq[ti1 * 8 + i] = q[i];
        } else {
#pragma unroll
          for (int l = 0; l < 3; ++l) s_pq[ti1 * 8 + 5 + l] = q[l];
        }
      }
    }
    DMX_WAVE_LDS_ORDER();
    if (!DIAG_ONLY && tid < 2 && slab == 0) {      // llks00: lane n adds its alpha's terms in pair order
      const double* row = &s_t00[tid * T00];
      for (int i = 0; i < tp; ++i) acc00 += row[i];
    }
    // ---- phase 2 in sub-tiles of SUB pairs
#pragma unroll 1
    for (int sub = 0; sub < tp; sub += SUB) {
      const int ns = min(SUB, tp - sub);
      const int buf = (sub / SUB) & 1;
      const float* s_g = s_g0 + buf * SUB * GSS;
      __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): this sub-tile's rows have landed ...
      if (sub + SUB < tp) request_rows(sub + SUB, buf ^ 1);   // ... the next one's take off (its buffer was last read two syncs ago)
      DMX_WAVE_LDS_ORDER();
#pragma unroll 1
      for (int pi = 0; pi < ns; ++pi) {                    // (two pairs per trip: 1 227.8 against 1 206.2 ms)
        const float* gr = &s_g[pi * GSS];
        const double* pq = &s_pq[(sub + pi) * 8];
        const double a[3] = {(double)gr[j * 3], (double)gr[j * 3 + 1], (double)gr[j * 3 + 2]};
        constexpr bool ROOMY = MINW <= 3;          // 168 registers: the pair's q values stay in registers, the next unit's row is read a unit ahead, the four logs interleave
        double Pr[5], Qr[3];
        if (ROOMY) {
#pragma unroll
          for (int c = 0; c < 5; ++c) Pr[c] = pq[c];
#pragma unroll
          for (int c = 0; c < 3; ++c) Qr[c] = pq[5 + c];
        }
        float bn[3] = {gr[kk[0] * 3], gr[kk[0] * 3 + 1], gr[kk[0] * 3 + 2]};
#pragma unroll
        for (int i = 0; i < (DIAG_ONLY ? 0 : NU); ++i) {
          const double b[3] = {(double)bn[0], (double)bn[1], (double)bn[2]};
          if (ROOMY && i + 1 < NU) { const int kn = kk[i + 1]; bn[0] = gr[kn * 3]; bn[1] = gr[kn * 3 + 1]; bn[2] = gr[kn * 3 + 2]; }
          else if (!ROOMY && i + 1 < NU) { const int kn = kk[i + 1]; bn[0] = gr[kn * 3]; bn[1] = gr[kn * 3 + 1]; bn[2] = gr[kn * 3 + 2]; }
          // two halves so that no more than the nine products, two sums and two logs are live at once (128 registers = four wavefronts per SIMD): first
          // the exact products E and the two alpha-0 entries, then E becomes T = E q[l + m] in place and serves the two alpha-0.5 entries
          double E[3][3];
#pragma unroll
          for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int m = 0; m < 3; ++m) E[l][m] = a[l] * b[m];                  // :553 (exact) — shared by [j][k] and [k][j] at both alphas
          {
            // [j][k][0]: l-major over (l, m) of (g_j[l] g_k[m]) q0[l]; [k][j][0]: of (g_k[l] g_j[m]) q0[l] = E[m][l] q0[l].  The first product initialises
            // the sum (0 + x == x for these non-negative products: the reference's bits, one add fewer).  (The pair's q values are re-read per half —
            // uniform LDS reads — instead of held across the pair's units: 16 registers the kernel does not have at four wavefronts per SIMD.)
            const double Q[3] = {ROOMY ? Qr[0] : lds_read_f64(&pq[5]), ROOMY ? Qr[1] : lds_read_f64(&pq[6]), ROOMY ? Qr[2] : lds_read_f64(&pq[7])};
            double s_jk0 = E[0][0] * Q[0], s_kj0 = E[0][0] * Q[0];
#pragma unroll
            for (int l = 0; l < 3; ++l)
#pragma unroll
              for (int m = 0; m < 3; ++m) {
                if (l == 0 && m == 0) continue;
                s_jk0 += (E[l][m] * Q[l]);
                s_kj0 += (E[m][l] * Q[l]);
              }
            acc[i][0] += dmx_log2_fast_pinned(s_jk0, s_log, lk);               // :683
            acc[i][2] += dmx_log2_fast_pinned(s_kj0, s_log, lk);
          }
          if (!ROOMY) __builtin_amdgcn_sched_barrier(0);
          {
            const double P[5] = {ROOMY ? Pr[0] : lds_read_f64(&pq[0]), ROOMY ? Pr[1] : lds_read_f64(&pq[1]), ROOMY ? Pr[2] : lds_read_f64(&pq[2]),
                                 ROOMY ? Pr[3] : lds_read_f64(&pq[3]), ROOMY ? Pr[4] : lds_read_f64(&pq[4])};
#pragma unroll
            for (int l = 0; l < 3; ++l)
#pragma unroll
              for (int m = 0; m < 3; ++m) E[l][m] = E[l][m] * P[l + m];         // T: :677-679 at alpha 0.5 — [k][j]'s nine terms are these, transposed
            double s_jk1 = E[0][0], s_kj1 = E[0][0];
#pragma unroll
            for (int l = 0; l < 3; ++l)
#pragma unroll
              for (int m = 0; m < 3; ++m) {
                if (l == 0 && m == 0) continue;
                s_jk1 += E[l][m];
                s_kj1 += E[m][l];
              }
            acc[i][1] += dmx_log2_fast_pinned(s_jk1, s_log, lk);
            acc[i][3] += dmx_log2_fast_pinned(s_kj1, s_log, lk);
          }
          __builtin_amdgcn_sched_barrier(0);       // one pair of entries at a time
        }
        if (slab == 0) {                           // the diagonal entry [j][j][h]
          double sd = 0.0;
#pragma unroll
          for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int m = 0; m < 3; ++m) {
              const double v = pq[5 + l + dg[m]];
              const double term = (a[l] * a[m]) * v;
              sd = (l == 0 && m == 0) ? term : sd + term;
            }
          accd += dmx_log2_fast_pinned(sd, s_log, lk);
        }
      }
      DMX_WAVE_LDS_ORDER();
    }
  }
  double* G = grid + (size_t)cell * V * V * A;
#pragma unroll
  for (int i = 0; i < (DIAG_ONLY ? 0 : NU); ++i) {
    const int d = 1 + 2 * (NU * slab + i) + h, k = kk[i];
    if (d < 16 || j < 16) {                        // d = 16 is reached from both sides: the j < 16 lane stores
      G[((size_t)j * V + k) * A] = acc[i][0]; G[((size_t)j * V + k) * A + 1] = acc[i][1];
      G[((size_t)k * V + j) * A] = acc[i][2]; G[((size_t)k * V + j) * A + 1] = acc[i][3];
    }
  }
  if (slab == 0) {
    G[((size_t)j * V + j) * A + h] = accd;
    if (!DIAG_ONLY && tid < 2) l00[(size_t)cell * A + tid] = acc00;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The diagonal of k_doublet_a2u's grid: entries [j][j][0..1] of 32 samples (STRICT, default grid).  Lane j of a barcode's 32 lanes owns BOTH alphas of its
// sample — the six distinct exact products g_j[l] g_j[m] once, two nine-term l-major sums, two logs, two accumulators — and a wavefront carries two barcodes
// (k_doublet_a2s<.., 0>, the first form, spent a 64-lane wavefront per barcode: lane (j, alpha), 62 instructions per pair; this one 83 per pair for two
// barcodes).  Per tile of 16 pairs and barcode: headers (16 lanes), phase 1 (32 lanes = pair x alpha; k_doublet_sym's, from the final-value table where
// every pair of the wavefront's two tiles is on it), then the lane's own three floats per pair straight from the matrix.  No workgroup barrier.
// LN: sample lanes per barcode — the whole panel, or (k_doublet_diag_lo, behind k_doublet_a2u2, which forms the entries of j = 16..31 itself) the first 16 samples
// of 32: four barcodes per wavefront, tiles of 8 pairs, rows still 96 floats apart.
template <int MINW, int VP, int LN>
__device__ __forceinline__ void diag_body(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                           const double* __restrict__ tabs, const int32_t* __restrict__ sched,
                                                           double* __restrict__ grid, const double* __restrict__ pfin, const double* __restrict__ pseed) {
  static_assert((VP == 32 || VP == 16) && (LN == VP || LN == 16), "panel");
  constexpr int V = VP, A = 2, TPC = LN, TP = LN / 2, CPW = kThreads / TPC, row_len = 3 * V, PB = 8, WPC = 64 / TPC;
  __shared__ double s_tab[kTab2];
  __shared__ double s_w[2][10];
  __shared__ __attribute__((aligned(16))) double s_pq_all[CPW][TP][8];
  __shared__ int64_t s_off_all[CPW][TP];
  __shared__ int32_t s_snp_all[CPW][TP];
  __shared__ uint32_t s_cnt_all[CPW][TP];
  const double* s_log = s_tab + kLut2;
  const int t = threadIdx.x;
  stage_k2_tables(s_tab, tabs, t, kThreads);
  if (t < 10) {
    const int n = t / 5, q = t % 5;
    const int l = n ? (q > 2 ? 2 : q) : min(q, 2), m = n ? q - l : 0;
    const double p = 0.5 * l + (m - l) * 0.5 * (n ? 0.5 : 0.0);
    s_w[n][q] = p;
    s_w[n][5 + q] = 1.0 - p;
  }
  __syncthreads();
  const int cw = t / TPC, tid = t % TPC;
  double* s_pq = &s_pq_all[cw][0][0];
  int64_t* s_off = s_off_all[cw]; int32_t* s_snp = s_snp_all[cw]; uint32_t* s_cnt = s_cnt_all[cw];
  const int slot = blockIdx.x * CPW + cw;
  if ((blockIdx.x * CPW + (cw & ~(WPC - 1))) >= pv.B) return;   // every barcode of the wavefront past the end (no workgroup barrier below)
  const bool cell_ok = slot < pv.B;
  const int32_t cell = cell_ok ? sched[slot] : 0;
  const int64_t p_beg = cell_ok ? pv.cell_pair_off[cell] : 0;
  const int64_t np = cell_ok ? pv.cell_pair_off[cell + 1] - p_beg : 0;
  int64_t rd_base = cell_ok ? pv.cell_read_off[cell] : 0;
  int64_t np_w = np;                               // the longer of the wavefront's two barcodes: the tile loop is wave-uniform
#pragma unroll
  for (int d = TPC; d < 64; d <<= 1) { const int64_t o = __shfl_xor(np_w, d); np_w = np_w > o ? np_w : o; }
  const int j = tid;
  double acc0 = 0.0, acc1 = 0.0;
  const DmxLogPins lk = dmx_log_pins();
  const int ti1 = tid >> 1, n1 = tid & 1;
  for (int64_t tbase = 0; tbase < np_w; tbase += TP) {
    const int tp = (int)max((int64_t)0, min((int64_t)TP, np - tbase));
    load_tile_headers<TP>(pv, nrd_width, p_beg, tbase, tp, tid, rd_base, s_cnt, s_off, s_snp);
    DMX_WAVE_LDS_ORDER();
    if (tp > 0) rd_base = s_off[tp - 1] + (int64_t)s_cnt[tp - 1];
    // ---- phase 1 (:597-663): lane (pair ti1, alpha n1), five distinct values
    {
      const bool on = ti1 < tp;
      const uint32_t cnt = on ? s_cnt[ti1] : 0u;
      const int64_t off = on ? s_off[ti1] : 0;
      const uint32_t rd4 = load_rd4(pv, off, cnt);
      double q[5];
      const int32_t fi = pfin ? certify_final_index(cnt, rd4) : -1;
      if (!__any(fi < 0)) {
        const double* fp = pfin + (size_t)fi * kCFinStride + (n1 ? 0 : 5);
        q[0] = fp[0]; q[1] = fp[1]; q[2] = fp[2];
        q[3] = n1 ? fp[3] : 0.0; q[4] = n1 ? fp[4] : 0.0;
      } else {
        double wA[5], wR[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) { wA[i] = s_w[n1][i]; wR[i] = s_w[n1][5 + i]; }
        certify_pair_values<5, false>(pv, cnt, off, rd4, s_tab, wA, wR, n1, q, pseed);
      }
      if (on) {
        if (n1) {
#pragma unroll
          for (int i = 0; i < 5; ++i) s_pq[ti1 * 8 + i] = q[i];
        } else {
#pragma unroll
          for (int l = 0; l < 3; ++l) s_pq[ti1 * 8 + 5 + l] = q[l];
        }
      }
    }
    DMX_WAVE_LDS_ORDER();
    // ---- phase 2: the lane's sample against itself, PB pairs' rows requested at once
#pragma unroll 1
    for (int sub = 0; sub < TP; sub += PB) {
      if (!__any(sub < tp)) break;
      float ar[PB][3];
#pragma unroll
      for (int pi = 0; pi < PB; ++pi) {
        const float* src = g + (size_t)s_snp[sub + pi] * row_len + j * 3;     // (entries past the tile's last pair hold SNP 0)
        ar[pi][0] = src[0]; ar[pi][1] = src[1]; ar[pi][2] = src[2];
      }
#pragma unroll
      for (int pi = 0; pi < PB; ++pi) {
        if (sub + pi < tp) {
          const double* pq = &s_pq[(sub + pi) * 8];
          const double a[3] = {(double)ar[pi][0], (double)ar[pi][1], (double)ar[pi][2]};
          const double P[5] = {pq[0], pq[1], pq[2], pq[3], pq[4]}, Q[3] = {pq[5], pq[6], pq[7]};
          double s0 = 0.0, s1 = 0.0;
#pragma unroll
          for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int m = 0; m < 3; ++m) {
              const double e = a[l] * a[m];                                   // :553 (exact; a[l] a[m] == a[m] a[l]: six distinct)
              const double t0 = e * Q[l], t1 = e * P[l + m];                  // :677-679 at alpha 0 (pG = q0[l]) and alpha 0.5 (pG = q1[l + m])
              s0 = (l == 0 && m == 0) ? t0 : s0 + t0;                         // l-major; the first product initialises the sum (0 + x == x)
              s1 = (l == 0 && m == 0) ? t1 : s1 + t1;
            }
          acc0 += dmx_log2_fast_pinned(s0, s_log, lk);                        // :683
          acc1 += dmx_log2_fast_pinned(s1, s_log, lk);
        }
      }
    }
    DMX_WAVE_LDS_ORDER();
  }
  if (cell_ok) {
    double* o = grid + (((size_t)cell * V + j) * V + j) * A;
    o[0] = acc0; o[1] = acc1;
  }
}
template <int MINW, int VP = 32>                // VP: the panel — 32 samples (two barcodes per wavefront) or 16 (four)
__global__ __launch_bounds__(kThreads, MINW) void k_doublet_diag(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                           const double* __restrict__ tabs, const int32_t* __restrict__ sched,
                                                           double* __restrict__ grid, const double* __restrict__ pfin, const double* __restrict__ pseed) {
  diag_body<MINW, VP, VP>(pv, nrd_width, g, tabs, sched, grid, pfin, pseed);
}
// ... of the samples j = 0..15 of 32 only (behind k_doublet_a2u2)
template <int MINW>
__global__ __launch_bounds__(kThreads, MINW) void k_doublet_diag_lo(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                           const double* __restrict__ tabs, const int32_t* __restrict__ sched,
                                                           double* __restrict__ grid, const double* __restrict__ pfin, const double* __restrict__ pseed) {
  diag_body<MINW, 32, 16>(pv, nrd_width, g, tabs, sched, grid, pfin, pseed);
}

// ---------------------------------------------------------------------------------------------------------------------
// K2 for alpha grids of 3..8 entries: k_doublet_a2's ownership, order and arithmetic with AP (= A rounded up to 2, 4 or 8)
// alphas per pair.  Phase 1 spreads the TP * AP (pair, alpha) lanes over all the cell's threads, in passes when the cell has
// fewer than that; the one-max-across-ALL-alphas renormalisation (:626-639) is a butterfly over the AP lanes of a pair.
// Phase 2 walks the alphas two at a time with their pG in registers, so an evaluation costs what it costs in k_doublet_a2.
template <int TPC, int NK, int AP>
__global__ __launch_bounds__(kThreads) void k_doublet_an(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                         const double* __restrict__ gp0, const double* __restrict__ tabs,
                                                         const double* __restrict__ alpha,
                                                         const int32_t* __restrict__ sched, int32_t V, int32_t A, int32_t GS,
                                                         double* __restrict__ grid, double* __restrict__ l00,
                                                         uint8_t* __restrict__ flagged) {
  static_assert(AP == 2 || AP == 4 || AP == 8, "alphas per pair padded to a power of two");
  constexpr int TP = 32;
  constexpr int CPW = kThreads / TPC;
  constexpr int T00 = TP + 2;
#define DMX_K2_SYNC() do { if (TPC == 64) { DMX_WAVE_LDS_ORDER(); } else { __syncthreads(); } } while (0)
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_tab[kTab2];
  const double* s_log = s_tab + kLut2;
  const int t = threadIdx.x;
  stage_k2_tables(s_tab, tabs, t, kThreads);
  __syncthreads();

  const int cw = t / TPC, tid = t % TPC;
  const size_t cell_bytes = (size_t)TP * AP * 9 * 8 + (size_t)TP * GS * 4 + (size_t)AP * T00 * 8 + TP * (4 + 4 + 8);
  unsigned char* base = s_raw + (size_t)cw * cell_bytes;
  double* s_pG = (double*)base;                                  // [TP][AP][9]
  float* s_g = (float*)(base + (size_t)TP * AP * 9 * 8);         // [TP][GS]
  double* s_t00 = (double*)((unsigned char*)s_g + (size_t)TP * GS * 4);   // [AP][T00]
  int64_t* s_off = (int64_t*)(s_t00 + AP * T00);                 // [TP]
  int32_t* s_snp = (int32_t*)(s_off + TP);                       // [TP]
  uint32_t* s_cnt = (uint32_t*)(s_snp + TP);                     // [TP]

  const int slot = blockIdx.x * CPW + cw;
  if (TPC == 64 && slot >= pv.B) return;
  const bool cell_ok = slot < pv.B;
  const int32_t cell = cell_ok ? sched[slot] : 0;
  const int64_t p_beg = cell_ok ? pv.cell_pair_off[cell] : 0;
  const int64_t np = cell_ok ? pv.cell_pair_off[cell + 1] - p_beg : 0;
  int64_t rd_base = cell_ok ? pv.cell_read_off[cell] : 0;

  const int KB = (V + NK - 1) / NK;
  const int JS = TPC / KB;
  const int jl = tid / KB, kb = tid % KB;
  const int j = (int)blockIdx.y * JS + jl;
  const bool owner = jl < JS && j < V;
  double acc[NK][AP];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk)
#pragma unroll
    for (int n = 0; n < AP; ++n) acc[kk][n] = 0.0;
  bool ok = true;
  double acc00 = 0.0;                            // lane tid < A owns llks00[tid]
  const int row_len = V * 3;
  constexpr int P1 = TP * AP;                    // phase-1 lanes per tile
  constexpr int NPASS = (P1 + TPC - 1) / TPC;
  const int n1 = tid % AP;                       // this thread's alpha in phase 1 (TPC is a multiple of AP)
  const bool n_ok = n1 < A;
  double wA[9], wR[9];
  {
    const double al = n_ok ? alpha[n1] : 0.0;
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const double p = 0.5 * l + (m - l) * 0.5 * al;                       // :613
        wA[l * 3 + m] = p;
        wR[l * 3 + m] = 1.0 - p;
      }
  }

  for (int64_t tbase = 0; tbase < np; tbase += TP) {
    const int tp = (int)min((int64_t)TP, np - tbase);
    load_tile_headers<TP>(pv, nrd_width, p_beg, tbase, tp, tid, rd_base, s_cnt, s_off, s_snp);
    DMX_K2_SYNC();
    rd_base = s_off[tp - 1] + (int64_t)s_cnt[tp - 1];
    stage_geno_rows<TPC>(g, s_snp, tp, tid, row_len, GS, s_g);
    // ---- phase 1: lane u = (pair u / AP, alpha u % AP)
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
      const int u = tid + pass * TPC;
      if (u >= P1) break;                          // uniform per wavefront (P1 and TPC are multiples of 64)
      const int ti1 = u / AP;
      const bool on = ti1 < tp && n_ok;
      const uint32_t cnt = (ti1 < tp) ? s_cnt[ti1] : 0u;
      const int64_t off = (ti1 < tp) ? s_off[ti1] : 0;
      double pG[9];
      const double mx = pair_values_open<9, AP, true, false>(pv, cnt, off, 0u, s_tab, wA, wR, n1, pG, nullptr, n_ok);
      if (on) {
        const double y = rcp_refined(mx);                                    // numerators >= 1e-6, mx in [1e-6, 1+1e-6]
        ok &= llks00_term(gp0, s_snp[ti1], [&](int l, int m) { const double v = div_by(pG[l * 3 + m], mx, y); s_pG[(ti1 * AP + n1) * 9 + l * 3 + m] = v; return v; },
                    s_log, &s_t00[n1 * T00 + ti1]);                      // :656-663 into the llks00 term
      }
    }
    DMX_K2_SYNC();
    if (tid < A) {                                 // llks00[n]: lane n adds its alpha's terms in pair order
      const double* row = &s_t00[tid * T00];
      for (int i = 0; i < tp; ++i) acc00 += row[i];
    }
    // ---- phase 2
    if (owner) {
      for (int ti = 0; ti < tp; ++ti) {
        const float* gr = &s_g[ti * GS];
        const double aj[3] = {(double)gr[j * 3], (double)gr[j * 3 + 1], (double)gr[j * 3 + 2]};
#pragma unroll
        for (int ap = 0; ap < AP / 2; ++ap) {
          if (2 * ap >= A) break;
          const double* P = &s_pG[(ti * AP + 2 * ap) * 9];
          if (2 * ap + 1 < A) {                    // two alphas share the nine products
            double P0[9], P1v[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) { P0[i] = P[i]; P1v[i] = P[9 + i]; }
#pragma unroll
            for (int kk = 0; kk < NK; ++kk) {
              const int k = min(kb * NK + kk, V - 1);
              const double bk[3] = {(double)gr[k * 3], (double)gr[k * 3 + 1], (double)gr[k * 3 + 2]};
              double s0 = 0.0, s1 = 0.0;                                      // :674
#pragma unroll
              for (int l = 0; l < 3; ++l)
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                  const double gp = aj[l] * bk[m];                            // :553 (exact)
                  s0 += (gp * P0[l * 3 + m]);                                 // :677-679, l-major
                  s1 += (gp * P1v[l * 3 + m]);
                }
              ok &= __builtin_amdgcn_class(s0, 0x100) && __builtin_amdgcn_class(s1, 0x100);
              acc[kk][2 * ap] += dmx_log2_fast(s0, s_log);                     // :683
              acc[kk][2 * ap + 1] += dmx_log2_fast(s1, s_log);
            }
          } else {                                 // the last alpha of an odd-sized grid
            double P0[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) P0[i] = P[i];
#pragma unroll
            for (int kk = 0; kk < NK; ++kk) {
              const int k = min(kb * NK + kk, V - 1);
              const double bk[3] = {(double)gr[k * 3], (double)gr[k * 3 + 1], (double)gr[k * 3 + 2]};
              double s0 = 0.0;
#pragma unroll
              for (int l = 0; l < 3; ++l)
#pragma unroll
                for (int m = 0; m < 3; ++m) s0 += ((aj[l] * bk[m]) * P0[l * 3 + m]);
              ok &= __builtin_amdgcn_class(s0, 0x100);
              acc[kk][2 * ap] += dmx_log2_fast(s0, s_log);
            }
          }
        }
      }
    }
    DMX_K2_SYNC();
  }
  if (cell_ok) {
    if (owner) {
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        const int k = kb * NK + kk;
        if (k < V) {
          double* o = grid + (((size_t)cell * V + j) * V + k) * A;
#pragma unroll
          for (int n = 0; n < AP; ++n) if (n < A) o[n] = acc[kk][n];
        }
      }
    }
    if (tid < A && blockIdx.y == 0) l00[(size_t)cell * A + tid] = acc00;
    if (!ok) flag_cell(flagged, cell);
  }
#undef DMX_K2_SYNC
}

// FAST mode for any alpha grid with alpha[0] == 0 (soft fields; the default grid {0, 0.5} has its own kernel, k_doublet_sym):
// k_doublet_an's ownership, phase 1 and accumulation order with the entry set demuxlet prints or decides on — the singlet column
// llksAB[j][0][0] and every (j, k) of the doublet alphas n >= 1 (cmd_cram_demuxlet.cpp:772-797,:799-814) — in the bilinear form
// g_j . (pG[n] g_k), u = pG[n] g_k formed once per (pair, n, k) in the LDS and shared by the V rows j.  llksAB[j][k != 0][0], which
// only the maxLLK scan reads (:713-721), is filled with llksAB[j][0][0].  A * V * V evaluations of 33.5 FP64 instructions become
// (A - 1) * V * V + V of 15.
template <int TPC, int NK, int AP, int VUS, int SUBP = 4, int MINW = 2, bool CHK = true>   // VUS: row stride of u in doubles (>= V + NK - 1,
                                                               // even): compile-time so that the reads use immediate offsets; CHK: see k_doublet_a2
__global__ __launch_bounds__(kThreads, MINW) void k_doublet_anf(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                         const double* __restrict__ gp0, const double* __restrict__ tabs,
                                                         const double* __restrict__ alpha,
                                                         const int32_t* __restrict__ sched, int32_t V, int32_t A, int32_t GS,
                                                         double* __restrict__ grid, double* __restrict__ l00,
                                                         uint8_t* __restrict__ flagged) {
  static_assert(AP == 2 || AP == 4 || AP == 8, "alphas per pair padded to a power of two");
  constexpr int TP = 32;
  constexpr int CPW = kThreads / TPC;
  constexpr int T00 = TP + 2;
#define DMX_K2_SYNC() do { if (TPC == 64) { DMX_WAVE_LDS_ORDER(); } else { __syncthreads(); } } while (0)
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_tab[kTab2];
  const double* s_log = s_tab + kLut2;
  const int t = threadIdx.x;
  stage_k2_tables(s_tab, tabs, t, kThreads);
  __syncthreads();

  const int cw = t / TPC, tid = t % TPC;
  constexpr int VU = VUS;
  const int NU = (A - 1) * 3 * VU + 4;           // doubles of u per pair: [n-1][l][k], then the alpha-0 u of sample 0 (3) + pad
  const size_t cell_bytes = (size_t)TP * AP * 9 * 8 + (size_t)TP * GS * 4 + (size_t)AP * T00 * 8 + TP * (4 + 4 + 8) +
                            (size_t)SUBP * NU * 8 + (size_t)TPC * 8;
  unsigned char* base = s_raw + (size_t)cw * cell_bytes;
  double* s_pG = (double*)base;                                  // [TP][AP][9]
  float* s_g = (float*)(base + (size_t)TP * AP * 9 * 8);         // [TP][GS]
  double* s_t00 = (double*)((unsigned char*)s_g + (size_t)TP * GS * 4);   // [AP][T00]
  int64_t* s_off = (int64_t*)(s_t00 + AP * T00);                 // [TP]
  int32_t* s_snp = (int32_t*)(s_off + TP);                       // [TP]
  uint32_t* s_cnt = (uint32_t*)(s_snp + TP);                     // [TP]
  double* s_u = (double*)(s_cnt + TP);                           // [SUBP][NU]
  double* s_sing = s_u + (size_t)SUBP * NU;                      // [TPC]  the singlet column at the end (row j -> its k-block threads)

  const int slot = blockIdx.x * CPW + cw;
  if (TPC == 64 && slot >= pv.B) return;
  const bool cell_ok = slot < pv.B;
  const int32_t cell = cell_ok ? sched[slot] : 0;
  const int64_t p_beg = cell_ok ? pv.cell_pair_off[cell] : 0;
  const int64_t np = cell_ok ? pv.cell_pair_off[cell + 1] - p_beg : 0;
  int64_t rd_base = cell_ok ? pv.cell_read_off[cell] : 0;

  const int KB = (V + NK - 1) / NK;
  const int JS = TPC / KB;
  const int jl = tid / KB, kb = tid % KB;
  const int j = (int)blockIdx.y * JS + jl;
  const bool owner = jl < JS && j < V;
  double acc[NK][AP - 1], accS = 0.0;            // [k of the block][alpha n >= 1]; accS: llksAB[j][0][0] (threads kb == 0)
#pragma unroll
  for (int kk = 0; kk < NK; ++kk)
#pragma unroll
    for (int n = 0; n < AP - 1; ++n) acc[kk][n] = 0.0;
  bool ok = true;
  const DmxLogPins lk = dmx_log_pins();
  double acc00 = 0.0;                            // lane tid < A owns llks00[tid]
  const int row_len = V * 3;
  constexpr int P1 = TP * AP;                    // phase-1 lanes per tile
  constexpr int NPASS = (P1 + TPC - 1) / TPC;
  const int n1 = tid % AP;                       // this thread's alpha in phase 1 (TPC is a multiple of AP)
  const bool n_ok = n1 < A;
  double wA[9], wR[9];
  {
    const double al = n_ok ? alpha[n1] : 0.0;
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const double p = 0.5 * l + (m - l) * 0.5 * al;                       // :613
        wA[l * 3 + m] = p;
        wR[l * 3 + m] = 1.0 - p;
      }
  }

  // (this kernel keeps its own copies of load_tile_headers, stage_geno_rows, pair_values_open and llks00_term: through the calls its AP = 8 forms
  //  spill a few registers more or fewer than before)
  for (int64_t tbase = 0; tbase < np; tbase += TP) {
    const int tp = (int)min((int64_t)TP, np - tbase);
    if (tid < TP) {
      const bool v = tid < tp;
      const uint32_t n = v ? load_nrd(pv.pair_nrd, p_beg + tbase + tid, nrd_width) : 0u;
      const uint32_t incl = seg_scan_incl<32>(n);
      s_cnt[tid] = n;
      s_off[tid] = rd_base + (int64_t)(incl - n);
      s_snp[tid] = v ? (pv.pair_snp ? pv.pair_snp[p_beg + tbase + tid] : (int32_t)(tbase + tid)) : 0;
    }
    DMX_K2_SYNC();
    rd_base = s_off[tp - 1] + (int64_t)s_cnt[tp - 1];
    {
      int r = tid % row_len, ti = tid / row_len;
      const int dr = TPC % row_len, dt = TPC / row_len;
      while (ti < tp) {
        s_g[ti * GS + r] = g[(size_t)s_snp[ti] * row_len + r];
        r += dr; ti += dt;
        if (r >= row_len) { r -= row_len; ++ti; }
      }
    }
    // ---- phase 1: lane u = (pair u / AP, alpha u % AP)
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
      const int u = tid + pass * TPC;
      if (u >= P1) break;                          // uniform per wavefront (P1 and TPC are multiples of 64)
      const int ti1 = u / AP;
      const bool on = ti1 < tp && n_ok;
      const uint32_t cnt = (ti1 < tp) ? s_cnt[ti1] : 0u;
      const int64_t off = (ti1 < tp) ? s_off[ti1] : 0;
      double pG[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) pG[i] = 1.0;                               // :597
      for (uint32_t r = 0; __any(r < cnt); ++r) {
        const bool live = r < cnt && n_ok;
        const uint32_t byte = (r < cnt) ? pv.reads[off + r] : 0u;
        const uint32_t bq = byte & 127u;
        const bool alt = (byte >> 7) != 0;
        const double pR = alt ? s_tab[128 + bq] : s_tab[bq];                // :606
        const double pA = alt ? s_tab[bq] : s_tab[128 + bq];                // :607
        double mx = 0.0;
        if (live) {
#pragma unroll
          for (int i = 0; i < 9; ++i) {
            pG[i] *= (pR * wR[i] + pA * wA[i]);                             // :625
            mx = fmax(mx, pG[i]);                                 // :626-627
          }
        }
#pragma unroll
        for (int d = 1; d < AP; d <<= 1) {                                  // one max across ALL alphas of the pair
          const double o = __shfl_xor(mx, d);
          mx = fmax(mx, o);
        }
        if (live) {
          if (cnt <= kSafeReads) {
            const double y = rcp_refined(mx);
#pragma unroll
            for (int i = 0; i < 9; ++i) pG[i] = div_by(pG[i], mx, y);       // :632-639
          } else {
#pragma unroll
            for (int i = 0; i < 9; ++i) pG[i] /= mx;
          }
        }
      }
      double mx = 0.0;
      if (n_ok) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          pG[i] += 1e-6;                                                     // :649
          mx = fmax(mx, pG[i]);
        }
      }
#pragma unroll
      for (int d = 1; d < AP; d <<= 1) {
        const double o = __shfl_xor(mx, d);
        mx = fmax(mx, o);
      }
      if (on) {
        const double y = rcp_refined(mx);
        const double* g0 = gp0 + (size_t)s_snp[ti1] * 3;
        const double qq[3] = {g0[0], g0[1], g0[2]};
        double sum = 0.0;
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            const double v = div_by(pG[l * 3 + m], mx, y);                   // :656-663
            s_pG[(ti1 * AP + n1) * 9 + l * 3 + m] = v;
            sum += ((qq[l] * qq[m]) * v);                                    // gp00 (:555) then :702-705
          }
        ok &= __builtin_amdgcn_class(sum, 0x100);
        s_t00[n1 * T00 + ti1] = dmx_log2_fast(sum, s_log);                    // :708-709 term
      }
    }
    DMX_K2_SYNC();
    if (tid < A) {                                 // llks00[n]: lane n adds its alpha's terms in pair order
      const double* row = &s_t00[tid * T00];
      for (int i = 0; i < tp; ++i) acc00 += row[i];
    }
    // ---- phase 2 in sub-tiles of SUBP pairs: u[n][l][k] = sum_m pG[n][l][m] g_k[m] once per (pair, n >= 1, k), then every printed
    //      entry is log(g_j . u_k) (bilinear form, fused multiply-adds)
#pragma unroll 1
    for (int sub = 0; sub < tp; sub += SUBP) {
      const int ns = min(SUBP, tp - sub);
      const int NI = (A - 1) * V + 1;              // items per pair: (n, k) for n >= 1, then the alpha-0 u of sample 0
#pragma unroll 1
      for (int e = tid; e < ns * NI; e += TPC) {
        const int pi = e / NI, it = e % NI;
        const bool sing = it == NI - 1;
        const int n = sing ? 0 : 1 + it / V, k = sing ? 0 : it % V;
        const double* P = &s_pG[((sub + pi) * AP + n) * 9];
        const float* gr = &s_g[(sub + pi) * GS + k * 3];
        const double b0 = (double)gr[0], b1 = (double)gr[1], b2 = (double)gr[2];
        double* u = sing ? &s_u[(size_t)pi * NU + (A - 1) * 3 * VU] : &s_u[(size_t)pi * NU + (size_t)(n - 1) * 3 * VU + k];
        const int us = sing ? 1 : VU;
#pragma unroll
        for (int l = 0; l < 3; ++l) u[l * us] = __builtin_fma(P[l * 3 + 2], b2, __builtin_fma(P[l * 3 + 1], b1, P[l * 3] * b0));
      }
      DMX_K2_SYNC();
      if (owner) {
        const int k0 = min(kb * NK, V - 1);
        const double* up = s_u + k0;               // this thread's first k; rows are VU apart, alphas 3 VU, pairs NU
#pragma unroll 1
        for (int pi = 0; pi < ns; ++pi, up += NU) {
          const float* gr = &s_g[(sub + pi) * GS];
          const double a0 = (double)gr[j * 3], a1 = (double)gr[j * 3 + 1], a2 = (double)gr[j * 3 + 2];
#pragma unroll
          for (int n = 1; n < AP; ++n) {
            if (n >= A) break;
#pragma unroll
            for (int kk = 0; kk < NK; ++kk) {
              // (k-blocks past the panel's end re-read its last columns: never stored)
              const int o = (n - 1) * 3 * VU + kk;
              const double x0 = lds_read_f64(&up[o]), x1 = lds_read_f64(&up[o + VU]), x2 = lds_read_f64(&up[o + 2 * VU]);
              const double sj = __builtin_fma(a2, x2, __builtin_fma(a1, x1, a0 * x0));
              if (CHK) ok &= __builtin_amdgcn_class(sj, 0x100) || kb * NK + kk >= V;
              acc[kk][n - 1] += dmx_log2_fastmode(sj, s_log, lk);
            }
            __builtin_amdgcn_sched_barrier(0);     // one alpha's NK evaluations in flight at a time (register budget)
          }
          if (kb == 0) {
            const double* u0 = s_u + (size_t)pi * NU + (A - 1) * 3 * VU;
            const double sj = __builtin_fma(a2, u0[2], __builtin_fma(a1, u0[1], a0 * u0[0]));
            ok &= __builtin_amdgcn_class(sj, 0x100);
            accS += dmx_log2_fastmode(sj, s_log, lk);
          }
        }
      }
      DMX_K2_SYNC();
    }
  }
  if (owner && kb == 0) s_sing[jl] = accS;
  DMX_K2_SYNC();
  if (cell_ok) {
    if (owner) {
      const double sj = s_sing[jl];                // llksAB[j][k != 0][0] is filled with llksAB[j][0][0]
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        const int k = kb * NK + kk;
        if (k < V) {
          double* o = grid + (((size_t)cell * V + j) * V + k) * A;
          o[0] = sj;
#pragma unroll
          for (int n = 1; n < AP; ++n) if (n < A) o[n] = acc[kk][n - 1];
        }
      }
    }
    if (tid < A && blockIdx.y == 0) l00[(size_t)cell * A + tid] = acc00;
    if (!ok) flag_cell(flagged, cell);
  }
#undef DMX_K2_SYNC
}

// ---------------------------------------------------------------------------------------------------------------------
// Genotype classes.  With --field GT every sample's probability row at a SNP is one of at most four float triplets
// (the three one-hot rows and the HWE row shared by all missing genotypes, bcf_filtered_reader.cpp:381-400), so
// log(sum_lm g_j[l] g_k[m] pG[l][m]) takes at most 16 distinct values per (pair, alpha) instead of V*V.  log and the
// arithmetic in front of it are pure functions of their operands: evaluating each distinct (class_j, class_k) once
// and adding the result into every accumulator that shares it is BIT-IDENTICAL to evaluating it V*V times, and keeps
// the per-accumulator addition order.  Rows are compared bitwise.  More than kMaxCls classes at any SNP (GP / PL
// inputs) => the class kernels are not used.
constexpr int kMaxCls = 4;

__global__ void k_build_classes(const float* __restrict__ g, int32_t S, int32_t V, float* __restrict__ rows /*[S][4][3]*/,
                                uint8_t* __restrict__ ids /*[S][V]*/, uint32_t* __restrict__ idw /*[S][ceil(V/16)] 2 bits per sample*/,
                                uint32_t* __restrict__ idd /*[S][nwd2]: word w = ids of samples (16 w + b) mod V, b = 0..15 (k_doublet_clsym)*/,
                                int32_t nwd2, int32_t* __restrict__ max_cls) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const uint32_t* gr = reinterpret_cast<const uint32_t*>(g + (size_t)s * V * 3);
  uint32_t c[kMaxCls][3];
  int n = 0;
  bool over = false;
  for (int32_t k = 0; k < V; ++k) {
    const uint32_t a0 = gr[k * 3], a1 = gr[k * 3 + 1], a2 = gr[k * 3 + 2];
    int id = -1;
    for (int d = 0; d < n; ++d) if (c[d][0] == a0 && c[d][1] == a1 && c[d][2] == a2) { id = d; break; }
    if (id < 0) {
      if (n < kMaxCls) { id = n; c[n][0] = a0; c[n][1] = a1; c[n][2] = a2; ++n; }
      else { over = true; id = 0; }
    }
    ids[(size_t)s * V + k] = (uint8_t)id;
  }
  const int nwd = (V + 15) / 16;
  for (int wq = 0; wq < nwd; ++wq) {
    uint32_t wv = 0;
    for (int b = 0; b < 16 && wq * 16 + b < V; ++b) wv |= (uint32_t)ids[(size_t)s * V + wq * 16 + b] << (2 * b);
    idw[(size_t)s * nwd + wq] = wv;
  }
  for (int wq = 0; wq < nwd2; ++wq) {
    uint32_t wv = 0;
    int k = (16 * wq) % V;
    for (int b = 0; b < 16; ++b) { wv |= (uint32_t)ids[(size_t)s * V + k] << (2 * b); k = (k + 1 == V) ? 0 : k + 1; }
    idd[(size_t)s * nwd2 + wq] = wv;
  }
  uint32_t* ro = reinterpret_cast<uint32_t*>(rows + (size_t)s * kMaxCls * 3);
  for (int d = 0; d < kMaxCls; ++d) {
    const int e = d < n ? d : 0;                 // unused classes repeat class 0 (never referenced by an id)
    ro[d * 3] = c[e][0]; ro[d * 3 + 1] = c[e][1]; ro[d * 3 + 2] = c[e][2];
  }
  atomicMax(max_cls, over ? kMaxCls + 1 : n);
}

// ---- canonical GT classes (round 4) ----------------------------------------------------------------------------------------------
// --field GT gives every called genotype one of THREE rows that do not depend on the SNP: 1 - gt_error in the genotype's place, gt_error / 2
// in the other two (bcf_filtered_reader.cpp:397-400); only a missing genotype's Hardy-Weinberg row (:381-388) is the SNP's own.  When a
// matrix has that shape the classes are relabelled: id t < 3 = the row with hi in place t, id 3 = the SNP's other row (at most one; the
// slot repeats canonical row 0 where there is none, like k_build_classes' unused slots).  log(GL . row_t) of a pair then depends on the
// pair's reads only, and K1 reads it from a table (k_build_canon_logs) next to the GL tables.
__device__ __forceinline__ bool canon_pattern(uint32_t a, uint32_t b, uint32_t c, uint32_t* hi, uint32_t* lo) {
  const float fa = __uint_as_float(a), fb = __uint_as_float(b), fc = __uint_as_float(c);
  if (!(fa >= 0.f && fb >= 0.f && fc >= 0.f) || !(fa < 3e38f && fb < 3e38f && fc < 3e38f)) return false;
  if (b == c && fa > fb) { *hi = a; *lo = b; return true; }
  if (a == c && fb > fa) { *hi = b; *lo = a; return true; }
  if (a == b && fc > fa) { *hi = c; *lo = a; return true; }
  return false;
}
__device__ __forceinline__ int canon_type(const uint32_t* r, uint32_t hi, uint32_t lo) {
  if (r[0] == hi && r[1] == lo && r[2] == lo) return 0;
  if (r[0] == lo && r[1] == hi && r[2] == lo) return 1;
  if (r[0] == lo && r[1] == lo && r[2] == hi) return 2;
  return -1;
}
// the lowest SNP that has a row of the pattern (its first such class names hi and lo: deterministic)
__global__ void k_find_canon(const float* __restrict__ rows, int32_t S, int32_t* __restrict__ first) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const uint32_t* r = reinterpret_cast<const uint32_t*>(rows + (size_t)s * kMaxCls * 3);
  uint32_t hi, lo;
  for (int d = 0; d < kMaxCls; ++d)
    if (canon_pattern(r[d * 3], r[d * 3 + 1], r[d * 3 + 2], &hi, &lo)) { atomicMin(first, (int32_t)s); return; }
}
// fail: an SNP with two different non-canonical rows among its classes
__global__ void k_canon_check(const float* __restrict__ rows, int32_t S, uint32_t hi, uint32_t lo, int32_t* __restrict__ fail) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const uint32_t* r = reinterpret_cast<const uint32_t*>(rows + (size_t)s * kMaxCls * 3);
  int others = 0; uint32_t o[3] = {0, 0, 0};
  for (int d = 0; d < kMaxCls; ++d) {
    const uint32_t* q = r + d * 3;
    if (canon_type(q, hi, lo) >= 0) continue;
    if (others && o[0] == q[0] && o[1] == q[1] && o[2] == q[2]) continue;       // (an unused slot repeating class 0)
    if (others) { atomicOr(fail, 1); return; }
    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; others = 1;
  }
}
__global__ void k_canon_apply(float* __restrict__ rows, uint8_t* __restrict__ ids, uint32_t* __restrict__ idw, uint32_t* __restrict__ idd,
                              int32_t S, int32_t V, int32_t nwd2, uint32_t hi, uint32_t lo, uint8_t* __restrict__ oth, int32_t* __restrict__ any_oth) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  uint32_t* r = reinterpret_cast<uint32_t*>(rows + (size_t)s * kMaxCls * 3);
  uint32_t map[kMaxCls], o[3] = {hi, lo, lo};
  bool has_other = false;
  for (int d = 0; d < kMaxCls; ++d) {
    const int t = canon_type(r + d * 3, hi, lo);
    if (t >= 0) map[d] = (uint32_t)t;
    else { map[d] = 3u; o[0] = r[d * 3]; o[1] = r[d * 3 + 1]; o[2] = r[d * 3 + 2]; has_other = true; }
  }
  bool used3 = false;
  for (int32_t k = 0; k < V; ++k) {
    const uint32_t id = map[ids[(size_t)s * V + k] & 3u];
    used3 |= id == 3u;
    ids[(size_t)s * V + k] = (uint8_t)id;
  }
  const int nwd = (V + 15) / 16;
  for (int wq = 0; wq < nwd; ++wq) {
    uint32_t wv = 0;
    for (int b = 0; b < 16 && wq * 16 + b < V; ++b) wv |= (uint32_t)ids[(size_t)s * V + wq * 16 + b] << (2 * b);
    idw[(size_t)s * nwd + wq] = wv;
  }
  for (int wq = 0; wq < nwd2; ++wq) {
    uint32_t wv = 0;
    int k = (16 * wq) % V;
    for (int b = 0; b < 16; ++b) { wv |= (uint32_t)ids[(size_t)s * V + k] << (2 * b); k = (k + 1 == V) ? 0 : k + 1; }
    idd[(size_t)s * nwd2 + wq] = wv;
  }
  r[0] = hi; r[1] = lo; r[2] = lo;  r[3] = lo; r[4] = hi; r[5] = lo;  r[6] = lo; r[7] = lo; r[8] = hi;
  r[9] = o[0]; r[10] = o[1]; r[11] = o[2];
  oth[s] = (has_other && used3) ? 1 : 0;
  if (has_other && used3) atomicOr(any_oth, 1);
}
// ltab[i][t] = log(GL_i . canonical row t), i over the final GL tables: 257 one-read entries (256 = no read), 16 384 two-read, 96^3 three-read
__global__ void k_build_canon_logs(const double* __restrict__ tabs, double hi, double lo, double* __restrict__ ltab) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kCanN) return;
  const double* G = i < kCanL2 ? tabs + kTab + kFirst + 3 * i
                  : (i < kCanL3 ? tabs + kTabK1 + kPair + 4 * (i - kCanL2) : tabs + kTabK1 + 2 * kPair + kTriple + 4 * (i - kCanL3));
  const double G0 = G[0], G1 = G[1], G2 = G[2];
  const double x0 = G0 * hi + G1 * lo + G2 * lo;      // the very expressions of k_singlet_cls on the canonical rows (:456)
  const double x1 = G0 * lo + G1 * hi + G2 * lo;
  const double x2 = G0 * lo + G1 * lo + G2 * hi;
  const double* T = tabs + kLut;
  ltab[4 * i] = dmx_log_fast(x0, T); ltab[4 * i + 1] = dmx_log_fast(x1, T); ltab[4 * i + 2] = dmx_log_fast(x2, T); ltab[4 * i + 3] = 0.0;
}

// K2 over genotype classes (A = 2).  Same ownership and order as k_doublet_a2; per tile of 32 pairs:
//   stage    headers, the pairs' class rows (4 x 3 float32) and per-sample class ids (V bytes) -> LDS
//   phase 1  pG[n][3][3] per (pair, alpha) and the llks00 term, exactly as k_doublet_a2
//   phase 1b the class table T[pair][cj][ck][n] = log(sum_lm row_cj[l] row_ck[m] pG[n][l][m]) — the very expression of
//            :553,:677-683 on the very operands, once per distinct (cj, ck)
//   phase 2  thread (j, k-block): acc[j][k][n] += T[pair][id_j][id_k][n], pairs in ascending SNP order
// UJ ("uniform j", panels of 33..64 samples): a wavefront owns a block of 16 samples j and its lanes are the samples k, so that the
// class of j is the same for the whole wavefront at every pair.  A lane reads its COLUMN T[0..3][ck] of the pair's table into sixteen
// consecutive registers and the row is chosen by VGPR-relative addressing (s_set_gpr_idx_on: the source register of the two v_add_f64
// is offset by 4 cj dwords) — no look-up, no address arithmetic and no branch per (j, k): two FP64 adds and two scalar instructions.
template <int TPC, int NK, int MINW = 1, bool UJ = false>
__global__ __launch_bounds__(kThreads, MINW) void k_doublet_cls(PileupView pv, int nrd_width, const float* __restrict__ rows,
                                                          const uint8_t* __restrict__ ids, const double* __restrict__ gp0,
                                                          const double* __restrict__ tabs, const double* __restrict__ alpha,
                                                          const int32_t* __restrict__ sched, int32_t V, int32_t VS,
                                                          double* __restrict__ grid, double* __restrict__ l00,
                                                          uint8_t* __restrict__ flagged) {
  constexpr int A = 2, TP = 32;
  constexpr int ablate = DMX_ABLATE;             // profiling builds only (tools/build_variant.sh); 0 in the product
  constexpr int CPW = kThreads / TPC;
  constexpr int T00 = TP + 2;
  constexpr int NT = kMaxCls * kMaxCls * A;      // class-table entries per pair
#define DMX_K2_SYNC() do { if (TPC == 64) { DMX_WAVE_LDS_ORDER(); } else { __syncthreads(); } } while (0)
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_tab[kTab2];
  __shared__ double s_w[2][18];                  // mixing weights of :613 per alpha (see k_doublet_a2): registers only while phase 1 runs
  const double* s_log = s_tab + kLut2;
  const int t = threadIdx.x;
  stage_k2_tables(s_tab, tabs, t, kThreads);
  if (t < 18) {
    const int n = t / 9, l = (t % 9) / 3, m = t % 3;
    const double p = 0.5 * l + (m - l) * 0.5 * alpha[n];
    s_w[n][t % 9] = p;
    s_w[n][9 + t % 9] = 1.0 - p;
  }
  __syncthreads();

  const int cw = t / TPC, tid = t % TPC;
  // The V > 32 form (NK = 16: 208 registers, 2 wavefronts per SIMD either way) runs a two-deep pipeline: while tile t computes,
  // the header of tile t + 2 and the class rows, ids, leading read bytes and gp0 of tile t + 1 are in flight into registers.
  // (panels of up to 64 samples: a tile's id words fit two registers per thread)
  constexpr bool PF_T = NK >= 16 && TPC == 256;
  const bool PF = PF_T && VS <= 64;
  const size_t cell_bytes = (size_t)TP * 18 * 8 + (size_t)TP * NT * 8 + 2 * T00 * 8 + TP * (4 + 4 + 8) + (size_t)TP * 12 * 4 + (size_t)TP * VS +
                            (PF_T ? (size_t)TP * 16 : 0);
  unsigned char* base = s_raw + (size_t)cw * ((cell_bytes + 15) & ~(size_t)15);
  double* s_pG = (double*)base;                                  // [TP][2][9]
  double* s_T = s_pG + TP * 18;                                  // [TP][4][4][2]
  double* s_t00 = s_T + TP * NT;                                 // [2][T00]
  int64_t* s_off = (int64_t*)(s_t00 + 2 * T00);                  // [TP]
  int32_t* s_snp = (int32_t*)(s_off + TP);                       // [TP]
  uint32_t* s_cnt = (uint32_t*)(s_snp + TP);                     // [TP]
  float* s_rows = (float*)(s_cnt + TP);                          // [TP][4][3]
  uint8_t* s_ids = (uint8_t*)(s_rows + TP * 12);                 // [TP][VS]
  int64_t* s_off2 = (int64_t*)(s_ids + (size_t)TP * VS);         // PF: [TP] header of the NEXT tile (VS is a multiple of 4, TP * VS of 128)
  int32_t* s_snp2 = (int32_t*)(s_off2 + TP);
  uint32_t* s_cnt2 = (uint32_t*)(s_snp2 + TP);

  const int slot = blockIdx.x * CPW + cw;
  if (TPC == 64 && slot >= pv.B) return;
  const bool cell_ok = slot < pv.B;
  const int32_t cell = cell_ok ? sched[slot] : 0;
  const int64_t p_beg = cell_ok ? pv.cell_pair_off[cell] : 0;
  const int64_t np = cell_ok ? pv.cell_pair_off[cell + 1] - p_beg : 0;
  int64_t rd_base = cell_ok ? pv.cell_read_off[cell] : 0;

  static_assert(!UJ || (TPC == 256 && NK == 16 && MINW <= 2), "the uniform-j form: four wavefronts x 16 samples j, 64 lanes = samples k; registers v[232:247] are its column");
  const int KB = (V + NK - 1) / NK;
  const int JS = TPC / KB;                       // rows per workgroup; more rows => j-slabs over blockIdx.y (see k_doublet_a2)
  const int jl = tid / KB, kb = tid % KB;
  const int j = (int)blockIdx.y * JS + jl;
  const int uj_k = tid & 63, uj_jb = tid >> 6;   // UJ: lane = sample k, wavefront = samples j in [16 uj_jb, 16 uj_jb + 16)
  const bool owner = UJ ? (uj_k < V && uj_jb * 16 < V) : (jl < JS && j < V);
  double acc[NK][A];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) { acc[kk][0] = 0.0; acc[kk][1] = 0.0; }
  bool ok = true;
  const int ti1 = tid >> 1, n1 = tid & 1;
  double acc00 = 0.0;

  constexpr int NRR = (TP * 12 + TPC - 1) / TPC, NRI = (TP * 16 + TPC - 1) / TPC;   // per-thread registers of a tile's rows / id words
  const int wpr = VS / 4;                        // id words per pair
  uint32_t hd_n = 0u; int32_t hd_s = 0;          // PF: header loads in flight (lanes < TP of the first wavefront)
  uint32_t pn = 0u; int32_t psn = 0; int64_t poff = 0;
  float d_rows[NRR]; uint32_t d_ids[NRI]; uint32_t d_rd4 = 0u; double d_g0[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < NRR; ++i) d_rows[i] = 0.f;
#pragma unroll
  for (int i = 0; i < NRI; ++i) d_ids[i] = 0u;
  auto load_hdr = [&](int64_t first) {
    hd_n = 0u; hd_s = 0;
    const int64_t nx = first + tid;
    if (tid < TP && nx < np) { hd_n = load_nrd(pv.pair_nrd, p_beg + nx, nrd_width); hd_s = pv.pair_snp ? pv.pair_snp[p_beg + nx] : (int32_t)nx; }
  };
  auto publish_next = [&]() {                    // first wavefront: hd_* (arrived) -> prepared header of the next tile, into LDS
    if (tid < 64) {
      pn = hd_n; psn = hd_s;
      const uint32_t incl = seg_scan_incl<32>(pn);
      poff = rd_base + (int64_t)(incl - pn);
      rd_base += (int64_t)__shfl(incl, 31);
      if (tid < TP) { s_cnt2[tid] = pn; s_off2[tid] = poff; s_snp2[tid] = psn; }
    }
  };
  auto request_next = [&]() {                    // everybody: the published tile's rows / ids (and read bytes, gp0) -> registers
#pragma unroll
    for (int i = 0; i < NRR; ++i) {
      const int e = tid + TPC * i;
      if (e < TP * 12) d_rows[i] = rows[(size_t)s_snp2[e / 12] * 12 + (e % 12)];
    }
#pragma unroll
    for (int i = 0; i < NRI; ++i) {
      const int e = tid + TPC * i;
      if (e < TP * wpr) {
        const int ti = e / wpr, wq = e % wpr;
        const uint8_t* src = ids + (size_t)s_snp2[ti] * V + wq * 4;
        uint32_t wv = 0;
        for (int b = 0; b < 4; ++b) if (wq * 4 + b < V) wv |= (uint32_t)src[b] << (8 * b);
        d_ids[i] = wv;
      }
    }
    if (tid < 64) {
      d_rd4 = load_rd4(pv, s_off2[ti1], s_cnt2[ti1]);
      const double* g0 = gp0 + (size_t)s_snp2[ti1] * 3;
      d_g0[0] = g0[0]; d_g0[1] = g0[1]; d_g0[2] = g0[2];
    }
  };
  if (PF) {
    load_hdr(0);
    publish_next();
    load_hdr(TP);
    __syncthreads();
    request_next();
    __syncthreads();                             // the next tile's header may be overwritten from here on
  }
  for (int64_t tbase = 0; tbase < np; tbase += TP) {
    const int tp = (int)min((int64_t)TP, np - tbase);
    uint32_t rd4_cur = 0u; double g0_cur[3] = {0.0, 0.0, 0.0};
    if (PF) {
      if (tid < TP) { s_cnt[tid] = pn; s_off[tid] = poff; s_snp[tid] = psn; }
#pragma unroll
      for (int i = 0; i < NRR; ++i) { const int e = tid + TPC * i; if (e < TP * 12) s_rows[e] = d_rows[i]; }
#pragma unroll
      for (int i = 0; i < NRI; ++i) { const int e = tid + TPC * i; if (e < TP * wpr) reinterpret_cast<uint32_t*>(s_ids)[e] = d_ids[i] << 4; }   // (ids staged as byte offsets of 16-byte table cells)
      rd4_cur = d_rd4; g0_cur[0] = d_g0[0]; g0_cur[1] = d_g0[1]; g0_cur[2] = d_g0[2];
      publish_next();
      load_hdr(tbase + 2 * TP);
      DMX_K2_SYNC();
      request_next();
    } else {
    load_tile_headers<TP>(pv, nrd_width, p_beg, tbase, tp, tid, rd_base, s_cnt, s_off, s_snp);
    DMX_K2_SYNC();
    rd_base = s_off[tp - 1] + (int64_t)s_cnt[tp - 1];
    // ---- class rows and ids -> LDS
    for (int e = tid; e < tp * 12; e += TPC) s_rows[e] = rows[(size_t)s_snp[e / 12] * 12 + (e % 12)];
    {
      for (int e = tid; e < tp * wpr; e += TPC) {
        const int ti = e / wpr, wq = e % wpr;
        const uint8_t* src = ids + (size_t)s_snp[ti] * V + wq * 4;
        uint32_t wv = 0;
        for (int b = 0; b < 4; ++b) if (wq * 4 + b < V) wv |= (uint32_t)src[b] << (8 * b);
        reinterpret_cast<uint32_t*>(s_ids)[ti * wpr + wq] = wv << 4;           // class id c (0..3) as c * 16: the byte offset of T[cj][c]
      }
    }
    }
    // ---- phase 1
    if (tid < 64 && !(ablate & 4096)) {
      const bool on = ti1 < tp;
      const uint32_t cnt = on ? s_cnt[ti1] : 0u;
      const int64_t off = on ? s_off[ti1] : 0;
      const uint32_t rd4 = PF ? rd4_cur : load_rd4(pv, off, cnt);   // the first four read bytes in one load (one dependent latency instead of four)
      // (its own copy of pair_values_open and llks00_term: through the calls k_doublet_cls<256, 16, 1, false> takes 253 registers instead of 252)
      double pG[9], wA[9], wR[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) { pG[i] = 1.0; wA[i] = s_w[n1][i]; wR[i] = s_w[n1][9 + i]; }
      for (uint32_t r = 0; __any(r < cnt); ++r) {
        const bool live = r < cnt;
        const uint32_t byte = live ? (r < 4 ? (rd4 >> (8 * r)) & 0xFFu : (uint32_t)pv.reads[off + r]) : 0u;
        const uint32_t bq = byte & 127u;
        const bool alt = (byte >> 7) != 0;
        const double pR = alt ? s_tab[128 + bq] : s_tab[bq];
        const double pA = alt ? s_tab[bq] : s_tab[128 + bq];
        double mx = 0.0;
        if (live) {
#pragma unroll
          for (int i = 0; i < 9; ++i) {
            pG[i] *= (pR * wR[i] + pA * wA[i]);
            mx = fmax(mx, pG[i]);
          }
        }
        {
          const double o = shfl_xor1(mx);
          mx = fmax(mx, o);
        }
        if (live) {
          if (cnt <= kSafeReads) {
            const double y = rcp_refined(mx);
#pragma unroll
            for (int i = 0; i < 9; ++i) pG[i] = div_by(pG[i], mx, y);
          } else {
#pragma unroll
            for (int i = 0; i < 9; ++i) pG[i] /= mx;
          }
        }
      }
      double mx = 0.0;
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        pG[i] += 1e-6;
        mx = fmax(mx, pG[i]);
      }
      {
        const double o = shfl_xor1(mx);
        mx = fmax(mx, o);
      }
      if (on) {
        const double y = rcp_refined(mx);
        const double* g0 = gp0 + (size_t)s_snp[ti1] * 3;
        const double qq[3] = {PF ? g0_cur[0] : g0[0], PF ? g0_cur[1] : g0[1], PF ? g0_cur[2] : g0[2]};
        double sum = 0.0;
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            const double v = div_by(pG[l * 3 + m], mx, y);
            s_pG[(ti1 * 2 + n1) * 9 + l * 3 + m] = v;
            sum += ((qq[l] * qq[m]) * v);
          }
        ok &= __builtin_amdgcn_class(sum, 0x100);
        s_t00[n1 * T00 + ti1] = dmx_log2_fast(sum, s_log);
      }
    }
    DMX_K2_SYNC();
    if (tid < 2) {
      const double* row = &s_t00[tid * T00];
      if (tp == TP) {                              // loads first (LDS latency paid once), then the ordered adds
        double2 v[TP / 2];
#pragma unroll
        for (int i = 0; i < TP / 2; ++i) v[i] = *reinterpret_cast<const double2*>(&row[2 * i]);
#pragma unroll
        for (int i = 0; i < TP / 2; ++i) { acc00 += v[i].x; acc00 += v[i].y; }
      } else {
        for (int i = 0; i < tp; ++i) acc00 += row[i];
      }
    }
    // ---- phase 1b: the class table
    for (int e = tid; e < ((ablate & 2048) ? 0 : tp * NT); e += TPC) {
      const int ti = e / NT, cc = e % NT;
      const int cj = cc >> 3, ck = (cc >> 1) & 3, n = cc & 1;
      const float* rj = &s_rows[ti * 12 + cj * 3];
      const float* rk = &s_rows[ti * 12 + ck * 3];
      const double* P = &s_pG[(ti * 2 + n) * 9];
      const double aj[3] = {(double)rj[0], (double)rj[1], (double)rj[2]};
      const double bk[3] = {(double)rk[0], (double)rk[1], (double)rk[2]};
      double sum = 0.0;                                                          // :674
#pragma unroll
      for (int l = 0; l < 3; ++l)
#pragma unroll
        for (int m = 0; m < 3; ++m) sum += ((aj[l] * bk[m]) * P[l * 3 + m]);     // :553, :677-679
      ok &= __builtin_amdgcn_class(sum, 0x100);
      s_T[ti * NT + cc] = dmx_log2_fast(sum, s_log);                              // the :683 term
    }
    DMX_K2_SYNC();
    // ---- phase 2: one lookup and two adds per (j, k)
    if (UJ) {
      if (owner && !(ablate & 1024)) {
        typedef uint32_t dmx_u4 __attribute__((ext_vector_type(4)));
        using lds_u4 = const __attribute__((address_space(3))) dmx_u4*;
        const uint32_t t_a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) double*)s_T;
        const uint32_t id_a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t*)s_ids;
        for (int ti = 0; ti < tp; ++ti) {
          // the 16 classes of the wavefront's samples j (bytes c * 16, one broadcast read) into scalar registers
          const dmx_u4 jw = *(lds_u4)(uintptr_t)(id_a + (uint32_t)(ti * VS + uj_jb * 16));
          const uint32_t w0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)jw.x), w1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)jw.y),
                         w2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)jw.z), w3 = (uint32_t)__builtin_amdgcn_readfirstlane((int)jw.w);
          // this lane's column of the pair's table: T[cj][ck] for cj = 0..3 (rows 64 bytes apart), ck = the class of sample k
          const uint32_t col = t_a + (uint32_t)(ti * NT * 8) + (uint32_t)s_ids[ti * VS + uj_k];
          // One asm statement per pair: the column into v[232:247] (T[c] = v[232 + 4c : 235 + 4c]: alpha 0, alpha 1), then per j
          // "index = 4 cj" (s_bfe_u32 takes bits 2..5 of the staged byte c * 16) and the two adds with SRC0 relative to it.
#define DMX_UJ_STEP(A0, A1, W, B)                                                                              \
          "s_bfe_u32 %[t], %[" W "], " B "\n\ts_set_gpr_idx_on %[t], 0x1\n\t"                                  \
          "v_add_f64 %[" A0 "], v[232:233], %[" A0 "]\n\tv_add_f64 %[" A1 "], v[234:235], %[" A1 "]\n\t"
          {
            uint32_t tmp;
            uint32_t m0_keep;                         // s_set_gpr_idx_on writes M0: saved and restored inside the statement (the
                                                      // compiler may keep an LDS-DMA base or a movrel index live in it)
            asm volatile(
                "s_mov_b32 %[m0k], m0\n\t"
                "ds_read_b128 v[232:235], %[col]\n\tds_read_b128 v[236:239], %[col] offset:64\n\t"
                "ds_read_b128 v[240:243], %[col] offset:128\n\tds_read_b128 v[244:247], %[col] offset:192\n\t"
                "s_waitcnt lgkmcnt(0)\n\t"
                DMX_UJ_STEP("a0", "b0", "w0", "0x40002") DMX_UJ_STEP("a1", "b1", "w0", "0x4000a")
                DMX_UJ_STEP("a2", "b2", "w0", "0x40012") DMX_UJ_STEP("a3", "b3", "w0", "0x4001a")
                DMX_UJ_STEP("a4", "b4", "w1", "0x40002") DMX_UJ_STEP("a5", "b5", "w1", "0x4000a")
                DMX_UJ_STEP("a6", "b6", "w1", "0x40012") DMX_UJ_STEP("a7", "b7", "w1", "0x4001a")
                DMX_UJ_STEP("a8", "b8", "w2", "0x40002") DMX_UJ_STEP("a9", "b9", "w2", "0x4000a")
                DMX_UJ_STEP("a10", "b10", "w2", "0x40012") DMX_UJ_STEP("a11", "b11", "w2", "0x4001a")
                DMX_UJ_STEP("a12", "b12", "w3", "0x40002") DMX_UJ_STEP("a13", "b13", "w3", "0x4000a")
                DMX_UJ_STEP("a14", "b14", "w3", "0x40012") DMX_UJ_STEP("a15", "b15", "w3", "0x4001a")
                "s_set_gpr_idx_off\n\ts_mov_b32 m0, %[m0k]"
                : [a0] "+v"(acc[0][0]), [b0] "+v"(acc[0][1]), [a1] "+v"(acc[1][0]), [b1] "+v"(acc[1][1]),
                  [a2] "+v"(acc[2][0]), [b2] "+v"(acc[2][1]), [a3] "+v"(acc[3][0]), [b3] "+v"(acc[3][1]),
                  [a4] "+v"(acc[4][0]), [b4] "+v"(acc[4][1]), [a5] "+v"(acc[5][0]), [b5] "+v"(acc[5][1]),
                  [a6] "+v"(acc[6][0]), [b6] "+v"(acc[6][1]), [a7] "+v"(acc[7][0]), [b7] "+v"(acc[7][1]),
                  [a8] "+v"(acc[8][0]), [b8] "+v"(acc[8][1]), [a9] "+v"(acc[9][0]), [b9] "+v"(acc[9][1]),
                  [a10] "+v"(acc[10][0]), [b10] "+v"(acc[10][1]), [a11] "+v"(acc[11][0]), [b11] "+v"(acc[11][1]),
                  [a12] "+v"(acc[12][0]), [b12] "+v"(acc[12][1]), [a13] "+v"(acc[13][0]), [b13] "+v"(acc[13][1]),
                  [a14] "+v"(acc[14][0]), [b14] "+v"(acc[14][1]), [a15] "+v"(acc[15][0]), [b15] "+v"(acc[15][1]),
                  [t] "=&s"(tmp), [m0k] "=&s"(m0_keep)
                : [col] "v"(col), [w0] "s"(w0), [w1] "s"(w1), [w2] "s"(w2), [w3] "s"(w3)
                : "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239", "v240", "v241", "v242", "v243", "v244", "v245",
                  "v246", "v247", "scc", "memory");
          }
#undef DMX_UJ_STEP
        }
      }
    } else
    if (owner) {
      for (int ti = 0; ti < tp; ++ti) {
        const uint8_t* idr = &s_ids[ti * VS];
        const int cj = idr[j] >> 4;
        const double* Tj = &s_T[ti * NT + cj * 8];
        typedef double dmx_d2v __attribute__((ext_vector_type(2)));
        using lds_c2 = const __attribute__((address_space(3))) dmx_d2v*;
        const uint32_t tj_a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) double*)Tj;   // LDS byte address of T[cj][0]
        if (NK >= 4) {                            // class ids of the k-block, four per 32-bit LDS read (VS is padded to 4)
#pragma unroll
          for (int kq = 0; kq < NK / 4; ++kq) {
            const uint32_t w4 = reinterpret_cast<const uint32_t*>(idr)[(kb * NK) / 4 + kq];
            // address = row + byte b of the id word: one v_add_u32 with an SDWA byte select (the ids were staged as c * 16)
            const dmx_d2v t0 = *(lds_c2)(uintptr_t)add_byte_of<0>(tj_a, w4), t1 = *(lds_c2)(uintptr_t)add_byte_of<1>(tj_a, w4),
                          t2 = *(lds_c2)(uintptr_t)add_byte_of<2>(tj_a, w4), t3 = *(lds_c2)(uintptr_t)add_byte_of<3>(tj_a, w4);
            acc[kq * 4 + 0][0] += t0.x; acc[kq * 4 + 0][1] += t0.y;             // :683, alpha 0 / alpha 1
            acc[kq * 4 + 1][0] += t1.x; acc[kq * 4 + 1][1] += t1.y;
            acc[kq * 4 + 2][0] += t2.x; acc[kq * 4 + 2][1] += t2.y;
            acc[kq * 4 + 3][0] += t3.x; acc[kq * 4 + 3][1] += t3.y;
          }
        } else {
#pragma unroll
          for (int kk = 0; kk < NK; ++kk) {
            const int k = min(kb * NK + kk, V - 1);
            const dmx_d2v tv = *(lds_c2)(uintptr_t)(tj_a + idr[k]);
            acc[kk][0] += tv.x;
            acc[kk][1] += tv.y;
          }
        }
      }
    }
    DMX_K2_SYNC();
  }
  if (cell_ok) {
    if (UJ) {
      if (owner) {
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
          const int jx = uj_jb * 16 + jj;
          if (jx < V) {
            double* o = grid + (((size_t)cell * V + jx) * V + uj_k) * A;
            o[0] = acc[jj][0]; o[1] = acc[jj][1];
          }
        }
      }
    } else
    if (owner) {
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        const int k = kb * NK + kk;
        if (k < V) {
          double* o = grid + (((size_t)cell * V + j) * V + k) * A;
          o[0] = acc[kk][0]; o[1] = acc[kk][1];
        }
      }
    }
    if (tid < 2 && blockIdx.y == 0) l00[(size_t)cell * A + tid] = acc00;
    if (!ok) flag_cell(flagged, cell);
  }
#undef DMX_K2_SYNC
}

// K2 over genotype classes, STRICT, A = 2, panels of 33..64 samples: PRODUCER / CONSUMER form of k_doublet_cls's uniform-j kernel (round 4).
// In k_doublet_cls a tile has four workgroup barriers and phase 1 runs on one of the barcode's four wavefronts while the other three
// wait (43 % of the wave time parked, rocprofv3 r03).  Here the four wavefronts of a barcode's workgroup have two roles:
//   wavefront 0 (producer)   tile t + 1: headers, class rows and ids (requested a tile ahead, in registers) -> LDS, phase 1 (pG, the
//                            llks00 terms and their ordered sum), phase 1b (the class table) into one half of a double buffer {T, ids};
//   wavefronts 1..3 (consumers)  tile t: phase 2 of the uniform-j form for 24 / 20 / 20 samples j — lanes = samples k, the pair's table
//                            column in sixteen consecutive registers, the row chosen by VGPR-relative addressing (see k_doublet_cls);
// ONE s_barrier per tile.  Phase 2 of a tile is ONE software-pipelined asm statement per wavefront (DMX_PJ_* below): while a pair's
// additions issue out of one set of column registers, the next pair's column is read into a second set and the class words of the pair
// after it into v[128:133] — no LDS round trip on the additions' path (the unpipelined loop of the round's first version had two per
// pair, about as long as the additions themselves: 741 ms at the cfg4 shard, this form 486 ms).  A wavefront's class words are simply
// its bytes of the pair's id row (class 0 beyond V): six or five aligned words.  Production (about 15 k cycles of one wavefront per tile,
// mostly latency) is as long as a consumer's 32 x 24 samples; with the last four samples j also on the producer (4 / 20 / 20 / 20, the
// first version) it was the critical path.  The consumers never touch global memory inside the loop: 168 registers, 3 wavefronts per SIMD
// (k_doublet_cls<256,16,uniform-j>: 256 registers, 2 per SIMD), so a SIMD has two other barcodes to issue for while one waits.
// Same operands, same operations, same order of additions as k_doublet_cls: bit-identical (tests).  cmd_cram_demuxlet.cpp:594-710.
constexpr int kPcJ1 = 24, kPcJ = 20;           // samples j of wavefront 1 and of wavefronts 2, 3
static_assert(kPcJ1 + 2 * kPcJ == 64 && kPcJ1 % 4 == 0 && kPcJ % 4 == 0, "k_doublet_clsp: a wavefront's class bytes are whole words of the id row");
// FAST (DMX_MODE_FAST, alpha grid {0, 0.5}; round 4): the same kernel over the entries demuxlet prints or decides on.  The class table holds
// alpha 0.5 only, ONE evaluation per unordered class pair (cj <= ck, mirrored: T is bitwise symmetric, so the accumulators of (j, k) and (k, j)
// add identical terms and the grid comes out mirrored without an exchange), plus the four alpha-0 values T[cj][class of sample 0] of the
// singlet column.  Phase 2 adds one value per (pair, j, k) instead of two (columns of 8 registers, index 16 + 2 c); the producer wavefront
// (lanes = samples j) accumulates the singlet column [j][0][0], which the never-printed [j][k][0] repeat (as in k_doublet_sym / _clsym).
// The values are STRICT's own (reference operation order) for the orientation evaluated.
template <int MINW, bool FAST = false>
__global__ __launch_bounds__(kThreads, MINW) void k_doublet_clsp(PileupView pv, int nrd_width, const float* __restrict__ rows,
                                                                const uint8_t* __restrict__ ids, const double* __restrict__ gp0,
                                                                const double* __restrict__ tabs, const double* __restrict__ alpha,
                                                                const int32_t* __restrict__ sched, int32_t V, int32_t VS,
                                                                double* __restrict__ grid, double* __restrict__ l00,
                                                                uint8_t* __restrict__ flagged) {
  constexpr int A = 2, TP = 32;
  constexpr int T00 = TP + 2;
  constexpr int NT = kMaxCls * kMaxCls * A;      // class-table entries per pair
  constexpr int VSC = 64;                        // id row stride in the LDS (bytes): compile-time for panels of up to 64 samples
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_tab[kTab2];
  __shared__ double s_w[2][18];                  // mixing weights of :613 per alpha
  const double* s_log = s_tab + kLut2;
  const int t = threadIdx.x;
  stage_k2_tables(s_tab, tabs, t, kThreads);
  if (t < 18) {
    const int n = t / 9, l = (t % 9) / 3, m = t % 3;
    const double p = 0.5 * l + (m - l) * 0.5 * alpha[n];
    s_w[n][t % 9] = p;
    s_w[n][9 + t % 9] = 1.0 - p;
  }
  // double-buffered (what phase 2 reads): the class table and the ids (as c * 16);
  // producer-private: pG, the llks00 terms, headers (current and next), rows
  double* s_Tb = (double*)s_raw;                                  // [2][TP][4][4][2]
  uint8_t* s_idb = (uint8_t*)(s_Tb + 2 * TP * NT);                // [2][TP][VSC]
  double* s_pG = (double*)(s_idb + 2 * (size_t)TP * VSC);         // [TP][2][9]
  double* s_t00 = s_pG + TP * 18;                                 // [2][T00]
  int64_t* s_off = (int64_t*)(s_t00 + 2 * T00);                   // [TP]
  int64_t* s_off2 = s_off + TP;                                   // [TP]  header of the NEXT tile
  int32_t* s_snp = (int32_t*)(s_off2 + TP);                       // [TP]
  int32_t* s_snp2 = s_snp + TP;
  uint32_t* s_cnt = (uint32_t*)(s_snp2 + TP);                     // [TP]
  uint32_t* s_cnt2 = s_cnt + TP;
  float* s_rows = (float*)(s_cnt2 + TP);                          // [TP][4][3]
  __syncthreads();

  const int32_t cell = sched[blockIdx.x];
  const int64_t p_beg = pv.cell_pair_off[cell];
  const int64_t np = pv.cell_pair_off[cell + 1] - p_beg;
  constexpr int wpr = VSC / 4;                   // id words per pair
  (void)VS;
  const int wave = t >> 6, lane = t & 63;        // lane = sample k in phase 2
  const int j0 = wave <= 1 ? 0 : kPcJ1 + (wave - 2) * kPcJ;      // first sample j of this (consumer) wavefront
  using lds_u8 = const __attribute__((address_space(3))) uint8_t*;

  // Phase 2 of one tile for a wavefront's samples j, one asm statement.  Per (pair, sample j): the class of j (wave-uniform) picks the row
  // of the lane's column by VGPR-relative addressing (see k_doublet_cls), then one addition per alpha.  Column sets X = v[152:167] and
  // Y = v[136:151] (the top of the 168-register budget), class words of the pair being requested in v[128:133], its id byte in v135;
  // two sets of class words in scalar registers (wa*, wb*).  Invariant at the top of a pair: its column requested, then the next pair's
  // words and id byte (NW LDS operations younger): s_waitcnt lgkmcnt(NW) is enough (LDS operations return in order).  The pairs beyond
  // the tile that the last rounds request read LDS inside the workgroup's allocation (the id byte is masked to a class's two bits, so the
  // column reads stay 16-byte aligned) and are drained before the statement ends.  DS instructions of gfx9+ do not use M0, so the
  // indexing state left in it is harmless; M0 is restored at the end.
  // The id bytes are 0x10 | c << 2 (FAST: 0x10 | c << 1): a word of four, shifted right by whole bytes, IS the M0 of the indexing mode —
  // M0[7:0] = 16 + 4 c (16 + 2 c; the column operands name the registers 16 below the set), M0[15:12] = the next byte's 0x1 = "index
  // SRC0".  One scalar instruction per sample j for three of a word's four (the hardware interlocks the M0 write against the indexed read).
  // Macro arguments: M = ST (STRICT: two additions per sample j, 16-register columns) | FA (FAST: one, 8-register columns); SET = SX | SY.
#define DMX_PJ_C0_SX "v[136:137]"
#define DMX_PJ_C1_SX "v[138:139]"
#define DMX_PJ_C0_SY "v[120:121]"
#define DMX_PJ_C1_SY "v[122:123]"
#define DMX_PJ_ADDS_ST(SET, A0, A1) "v_add_f64 %[" A0 "], " DMX_PJ_C0_##SET ", %[" A0 "]\n\tv_add_f64 %[" A1 "], " DMX_PJ_C1_##SET ", %[" A1 "]\n\t"
#define DMX_PJ_ADDS_FA(SET, A0, A1) "v_add_f64 %[" A1 "], " DMX_PJ_C0_##SET ", %[" A1 "]\n\t"
#define DMX_PJ_WORD4(M, SET, W, A0, B0, A1, B1, A2, B2, A3, B3)                                                     \
  "s_set_gpr_idx_on %[" W "], 0x1\n\t" DMX_PJ_ADDS_##M(SET, A0, B0)                                                \
  "s_lshr_b32 m0, %[" W "], 8\n\t" DMX_PJ_ADDS_##M(SET, A1, B1)                                                    \
  "s_lshr_b32 m0, %[" W "], 16\n\t" DMX_PJ_ADDS_##M(SET, A2, B2)                                                   \
  "s_lshr_b32 %[t], %[" W "], 24\n\ts_set_gpr_idx_on %[t], 0x1\n\t" DMX_PJ_ADDS_##M(SET, A3, B3)
#define DMX_PJ_FIRST4(M, SET, P) DMX_PJ_WORD4(M, SET, P "0", "a0", "b0", "a1", "b1", "a2", "b2", "a3", "b3")
#define DMX_PJ_REST16(M, SET, P)                                                                                  \
  DMX_PJ_WORD4(M, SET, P "1", "a4", "b4", "a5", "b5", "a6", "b6", "a7", "b7")                                       \
  DMX_PJ_WORD4(M, SET, P "2", "a8", "b8", "a9", "b9", "a10", "b10", "a11", "b11")                                   \
  DMX_PJ_WORD4(M, SET, P "3", "a12", "b12", "a13", "b13", "a14", "b14", "a15", "b15")                               \
  DMX_PJ_WORD4(M, SET, P "4", "a16", "b16", "a17", "b17", "a18", "b18", "a19", "b19")
#define DMX_PJ_REST20(M, SET, P) DMX_PJ_REST16(M, SET, P)                                                          \
  DMX_PJ_WORD4(M, SET, P "5", "a20", "b20", "a21", "b21", "a22", "b22", "a23", "b23")
  // the lane's column of the pair's table: T[cj][ck][n] for cj = 0..3 (rows 64 bytes apart), ck = the class of sample k = lane
#define DMX_PJ_COLADDR_ST "v_and_b32 %[colv], 12, v135\n\tv_lshl_add_u32 %[colv], %[colv], 2, %[pt]\n\t"
#define DMX_PJ_COLADDR_FA "v_and_b32 %[colv], 6, v135\n\tv_lshl_add_u32 %[colv], %[colv], 3, %[pt]\n\t"
#define DMX_PJ_READS_ST_SX "ds_read_b128 v[152:155], %[colv]\n\tds_read_b128 v[156:159], %[colv] offset:64\n\t"                                     \
                           "ds_read_b128 v[160:163], %[colv] offset:128\n\tds_read_b128 v[164:167], %[colv] offset:192\n\t"
#define DMX_PJ_READS_ST_SY "ds_read_b128 v[136:139], %[colv]\n\tds_read_b128 v[140:143], %[colv] offset:64\n\t"                                     \
                           "ds_read_b128 v[144:147], %[colv] offset:128\n\tds_read_b128 v[148:151], %[colv] offset:192\n\t"
  // (FAST: the alpha-0.5 halves only; offsets in 8-byte units)
#define DMX_PJ_READS_FA_SX "ds_read2_b64 v[152:155], %[colv] offset0:1 offset1:9\n\tds_read2_b64 v[156:159], %[colv] offset0:17 offset1:25\n\t"
#define DMX_PJ_READS_FA_SY "ds_read2_b64 v[136:139], %[colv] offset0:1 offset1:9\n\tds_read2_b64 v[140:143], %[colv] offset0:17 offset1:25\n\t"
  // the next pair: wait for its words / id byte, request its column into the set and move its words into a scalar set (RFL); then
  // request the words of the pair after it (WORDS).  pj: the wavefront's words in the id row, pi: the lane's id byte, pt: the table.
#define DMX_PJ_MID(M, SET, RFL, WORDS)                                                                            \
  "s_set_gpr_idx_off\n\ts_waitcnt lgkmcnt(0)\n\t" DMX_PJ_COLADDR_##M DMX_PJ_READS_##M##_##SET RFL                   \
  "v_add_u32 %[pj], 64, %[pj]\n\tv_add_u32 %[pi], 64, %[pi]\n\tv_add_u32 %[pt], 0x100, %[pt]\n\t"                   \
  WORDS
#define DMX_PJ_WORDS5 "ds_read2_b32 v[128:129], %[pj] offset1:1\n\tds_read2_b32 v[130:131], %[pj] offset0:2 offset1:3\n\t" \
                      "ds_read_b32 v132, %[pj] offset:16\n\tds_read_u8 v135, %[pi]\n\t"
#define DMX_PJ_WORDS6 "ds_read2_b32 v[128:129], %[pj] offset1:1\n\tds_read2_b32 v[130:131], %[pj] offset0:2 offset1:3\n\t" \
                      "ds_read2_b32 v[132:133], %[pj] offset0:4 offset1:5\n\tds_read_u8 v135, %[pi]\n\t"
#define DMX_PJ_RFL5(Q)                                                                                            \
  "v_readfirstlane_b32 %[" Q "0], v128\n\tv_readfirstlane_b32 %[" Q "1], v129\n\tv_readfirstlane_b32 %[" Q "2], v130\n\t" \
  "v_readfirstlane_b32 %[" Q "3], v131\n\tv_readfirstlane_b32 %[" Q "4], v132\n\t"
#define DMX_PJ_RFL6(Q) DMX_PJ_RFL5(Q) "v_readfirstlane_b32 %[" Q "5], v133\n\t"
  // a consumer's tile: WORDS / RFL(set) / REST for its 20 or 24 samples j.  At the top of a pair its column is requested and then the
  // next pair's words and id byte, four LDS operations younger: s_waitcnt lgkmcnt(4) waits for exactly the column.
#define DMX_PJ_CONSUMER(M, WORDS, RFL, REST)                                                                       \
  "s_mov_b32 %[m0k], m0\n\t" WORDS DMX_PJ_MID(M, SX, RFL("wa"), WORDS) "s_mov_b32 %[ti], 0\n"                      \
  "L_pjc_%=:\n\t"                                                                                                 \
  "s_waitcnt lgkmcnt(4)\n\t" DMX_PJ_FIRST4(M, SX, "wa") DMX_PJ_MID(M, SY, RFL("wb"), WORDS)                        \
  REST(M, SX, "wa") DMX_PJ_NEXT("L_pjd_%=")                                                                       \
  "s_waitcnt lgkmcnt(4)\n\t" DMX_PJ_FIRST4(M, SY, "wb") DMX_PJ_MID(M, SX, RFL("wa"), WORDS)                        \
  REST(M, SY, "wb")                                                                                               \
  "s_add_u32 %[ti], %[ti], 1\n\ts_cmp_lt_u32 %[ti], %[tp]\n\ts_cbranch_scc1 L_pjc_%=\n"                           \
  "L_pjd_%=:\n\t" DMX_PJ_END
#define DMX_PJ_NEXT(LBL) "s_add_u32 %[ti], %[ti], 1\n\ts_cmp_ge_u32 %[ti], %[tp]\n\ts_cbranch_scc1 " LBL "\n\t"
#define DMX_PJ_END "s_set_gpr_idx_off\n\ts_waitcnt lgkmcnt(0)\n\ts_mov_b32 m0, %[m0k]"
#define DMX_PJ_CLOB "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v142", "v143", "v144", \
                    "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159", \
                    "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167", "scc", "memory"

  // FAST, phase 1b: the class table of tile [tbase, ..) into buffer b2, by ALL FOUR wavefronts between two barriers of their own (14 of 16
  // slots per pair, two per thread): in FAST the producer is the longer role (phase 2 is half of STRICT's), and its 1b was half of its time.
  auto phase1b_fast = [&](int64_t tbase, int b2, bool& ok) {
    const int tp = (int)min((int64_t)TP, np - tbase);
    double* s_T = s_Tb + (size_t)b2 * TP * NT;
    const uint8_t* s_ids = s_idb + (size_t)b2 * TP * VSC;
    const int q = t & 15;
    // q < 10: the unordered class pairs (cj <= ck) at alpha 0.5; q = 10..13: (cj = q - 10, the class of sample 0) at alpha 0
    const int cj = (0xE4E9500u >> (2 * q)) & 3, ckq = (0xFB9E4u >> (2 * q)) & 3, n = q < 10 ? 1 : 0;
    if (q < 14)
      for (int ti = t >> 4; ti < tp; ti += kThreads / 16) {
        const int ck = q < 10 ? ckq : (s_ids[ti * VSC] >> 1) & 3;
        const float* rj = &s_rows[ti * 12 + cj * 3];
        const float* rk = &s_rows[ti * 12 + ck * 3];
        const double* P = &s_pG[(ti * 2 + n) * 9];
        const double aj[3] = {(double)rj[0], (double)rj[1], (double)rj[2]};
        const double bk[3] = {(double)rk[0], (double)rk[1], (double)rk[2]};
        double sum = 0.0;                                                          // :674
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) sum += ((aj[l] * bk[m]) * P[l * 3 + m]);     // :553, :677-679
        ok &= __builtin_amdgcn_class(sum, 0x100);
        const double val = dmx_log2_fast(sum, s_log);                              // the :683 term
        s_T[ti * NT + (cj * 4 + ck) * 2 + n] = val;
        if (q < 10) s_T[ti * NT + (ck * 4 + cj) * 2 + 1] = val;
      }
  };

  if (wave == 0) {
    // ================================================= producer =================================================
    const int ti1 = lane >> 1, n1 = lane & 1;
    int64_t rd_base = pv.cell_read_off[cell];
    double acc00 = 0.0;
    [[maybe_unused]] double acc0 = 0.0;          // FAST: the singlet column entry of sample j = lane
    bool ok = true;
    constexpr int NRR = 6, NRI = 8;              // per-lane registers of a tile's rows / id words: half a pair's 12 floats / 16 id words
    uint32_t hd_n = 0u; int32_t hd_s = 0;        // header loads in flight (lanes < TP)
    uint32_t pn = 0u; int32_t psn = 0; int64_t poff = 0;
    float d_rows[NRR]; uint32_t d_ids[NRI]; uint32_t d_rd4 = 0u; double d_g0[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < NRR; ++i) d_rows[i] = 0.f;
#pragma unroll
    for (int i = 0; i < NRI; ++i) d_ids[i] = 0u;
    auto load_hdr = [&](int64_t first) {
      hd_n = 0u; hd_s = 0;
      const int64_t nx = first + lane;
      if (lane < TP && nx < np) { hd_n = load_nrd(pv.pair_nrd, p_beg + nx, nrd_width); hd_s = pv.pair_snp ? pv.pair_snp[p_beg + nx] : (int32_t)nx; }
    };
    auto publish_next = [&]() {                  // hd_* (arrived) -> the prepared header of the next tile, into LDS
      pn = hd_n; psn = hd_s;
      const uint32_t incl = seg_scan_incl<32>(pn);
      poff = rd_base + (int64_t)(incl - pn);
      rd_base += (int64_t)__shfl(incl, 31);
      if (lane < TP) { s_cnt2[lane] = pn; s_off2[lane] = poff; s_snp2[lane] = psn; }
    };
    auto request_next = [&]() {                  // the published tile's rows, ids, leading read bytes and gp0 -> registers
      // lane (pair ti1, half n1): six consecutive floats of the pair's class rows and eight consecutive id words — one base address each
      const int32_t snp = s_snp2[ti1];
      const float* rsrc = rows + (size_t)snp * 12 + n1 * 6;
#pragma unroll
      for (int i = 0; i < NRR; ++i) d_rows[i] = rsrc[i];
      const uint8_t* isrc = ids + (size_t)snp * V + n1 * 32;
#pragma unroll
      for (int i = 0; i < NRI; ++i) {
        // one (possibly unaligned) 4-byte load per word: gfx950 global loads take any alignment; a row's last word is masked to its V
        // bytes (the bytes beyond belong to the next SNP's row; d_ids is allocated with 16 bytes of slack)
        const int k0 = n1 * 32 + 4 * i;
        uint32_t wv = 0;
        if (k0 < V) {
          __builtin_memcpy(&wv, isrc + 4 * i, 4);
          const int nb = V - k0;
          if (nb < 4) wv &= (1u << (8 * nb)) - 1u;
        }
        d_ids[i] = wv;
      }
      d_rd4 = load_rd4(pv, s_off2[ti1], s_cnt2[ti1]);
      const double* g0 = gp0 + (size_t)snp * 3;
      d_g0[0] = g0[0]; d_g0[1] = g0[1]; d_g0[2] = g0[2];
    };
    auto build = [&](int64_t tbase, int b) {     // tile [tbase, tbase + TP) -> buffer b
      const int tp = (int)min((int64_t)TP, np - tbase);
      double* s_T = s_Tb + (size_t)b * TP * NT;
      uint8_t* s_ids = s_idb + (size_t)b * TP * VSC;
      if (lane < TP) { s_cnt[lane] = pn; s_off[lane] = poff; s_snp[lane] = psn; }
#pragma unroll
      for (int i = 0; i < NRR; ++i) s_rows[ti1 * 12 + n1 * 6 + i] = d_rows[i];
#pragma unroll
      for (int i = 0; i < NRI; ++i) reinterpret_cast<uint32_t*>(s_ids)[ti1 * wpr + n1 * 8 + i] =
          (d_ids[i] << (FAST ? 1 : 2)) | 0x10101010u;                    // class id c as 0x10 | c << 2 (FAST: 0x10 | c << 1), see DMX_PJ_WORD4
      const uint32_t rd4 = d_rd4;
      const double qq[3] = {d_g0[0], d_g0[1], d_g0[2]};
      publish_next();
      load_hdr(tbase + 2 * TP);
      DMX_WAVE_LDS_ORDER();
      // ---- phase 1
      {
        const bool on = ti1 < tp;
        const uint32_t cnt = on ? s_cnt[ti1] : 0u;
        const int64_t off = on ? s_off[ti1] : 0;
        double pG[9];
        const double mx = pair_values_open<9, 2, true>(pv, cnt, off, rd4, s_tab, &s_w[n1][0], &s_w[n1][9], n1, pG);   // (the weights stay in LDS)
        if (on) {
          const double y = rcp_refined(mx);
          ok &= llks00_term(qq, [&](int l, int m) { const double v = div_by(pG[l * 3 + m], mx, y); s_pG[(ti1 * 2 + n1) * 9 + l * 3 + m] = v; return v; },
                      s_log, &s_t00[n1 * T00 + ti1]);
        }
      }
      DMX_WAVE_LDS_ORDER();
      request_next();                                              // (after phase 1: its registers are free again; phase 1b, this wavefront's
                                                                   //  phase 2 and the barrier cover the loads' latency)
      if (lane < 2) {
        const double* row = &s_t00[lane * T00];
        if (tp == TP) {                              // loads first (LDS latency paid once), then the ordered adds
          double2 v[TP / 2];
#pragma unroll
          for (int i = 0; i < TP / 2; ++i) v[i] = *reinterpret_cast<const double2*>(&row[2 * i]);
#pragma unroll
          for (int i = 0; i < TP / 2; ++i) { acc00 += v[i].x; acc00 += v[i].y; }
        } else {
          for (int i = 0; i < tp; ++i) acc00 += row[i];
        }
      }
      // ---- phase 1b: the class table (16 entries per lane; FAST: 14 of 16 slots per pair, 8 per lane)
      if constexpr (!FAST)
      for (int e = lane; e < tp * NT; e += 64) {
        const int ti = e / NT, cc = e % NT;
        const int cj = cc >> 3, ck = (cc >> 1) & 3, n = cc & 1;
        const float* rj = &s_rows[ti * 12 + cj * 3];
        const float* rk = &s_rows[ti * 12 + ck * 3];
        const double* P = &s_pG[(ti * 2 + n) * 9];
        const double aj[3] = {(double)rj[0], (double)rj[1], (double)rj[2]};
        const double bk[3] = {(double)rk[0], (double)rk[1], (double)rk[2]};
        double sum = 0.0;                                                          // :674
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) sum += ((aj[l] * bk[m]) * P[l * 3 + m]);     // :553, :677-679
        ok &= __builtin_amdgcn_class(sum, 0x100);
        s_T[ti * NT + cc] = dmx_log2_fast(sum, s_log);                              // the :683 term
      }
      DMX_WAVE_LDS_ORDER();                                        // (pG, t00, rows and the headers are rewritten by the next build)
    };
    if (np > 0) {
      load_hdr(0);
      publish_next();
      load_hdr(TP);
      DMX_WAVE_LDS_ORDER();
      request_next();
      DMX_WAVE_LDS_ORDER();                        // (the next tile's header may be overwritten from here on)
    }
    int b = 1;                                     // the round before the first tile only builds tile 0 (into buffer 0)
    for (int64_t tbase = -TP; tbase < np; tbase += TP, b ^= 1) {
      if (tbase + TP < np) build(tbase + TP, b ^ 1);
      if constexpr (FAST) {
        if (tbase >= 0) {                          // the singlet column [j][0][0] of tile t: lanes = samples j (class 0 beyond V: unused sums)
          const int tp = (int)min((int64_t)TP, np - tbase);
          const uint8_t* s_ids = s_idb + (size_t)b * TP * VSC;
          const double* s_T = s_Tb + (size_t)b * TP * NT;
#pragma unroll 8
          for (int ti = 0; ti < tp; ++ti) {
            const int cj = (s_ids[ti * VSC + lane] >> 1) & 3, c0 = (s_ids[ti * VSC] >> 1) & 3;
            acc0 += s_T[ti * NT + (cj * 4 + c0) * 2];
          }
        }
      }
      __syncthreads();
      if constexpr (FAST) {
        if (tbase + TP < np) phase1b_fast(tbase + TP, b ^ 1, ok);
        __syncthreads();
      }
    }
    if constexpr (FAST) {
      s_pG[lane] = acc0;                           // (pG is the producer's own and idle now) -> the consumers' rows
      __syncthreads();
    }
    if (lane < 2) l00[(size_t)cell * A + lane] = acc00;
    if (!ok) flag_cell(flagged, cell);
  } else {
    // ================================================= consumers ================================================
    const bool owner = lane < V && j0 < V;
    [[maybe_unused]] bool ok = true;               // (FAST: this wavefront's share of phase 1b)
    constexpr int NJM = kPcJ1;
    const int nj = wave == 1 ? kPcJ1 : kPcJ;
    double acc[NJM][A];
#pragma unroll
    for (int kk = 0; kk < NJM; ++kk) { acc[kk][0] = 0.0; acc[kk][1] = 0.0; }
    int b = 1;
    for (int64_t tbase = -TP; tbase < np; tbase += TP, b ^= 1) {
      const int tp = tbase < 0 ? 0 : (int)min((int64_t)TP, np - tbase);
      if (owner && tp > 0) {
        const uint8_t* s_ids = s_idb + (size_t)b * TP * VSC;
        uint32_t pi = (uint32_t)(uintptr_t)(lds_u8)(s_ids + lane), pj = (uint32_t)(uintptr_t)(lds_u8)(s_ids + j0);
        uint32_t pt = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) double*)(s_Tb + (size_t)b * TP * NT);
        uint32_t tmp, m0_keep, colv, ti_c, wa0, wa1, wa2, wa3, wa4, wb0, wb1, wb2, wb3, wb4;
        if (wave == 1) {
          uint32_t wa5, wb5;
          if constexpr (FAST) {
            asm volatile(DMX_PJ_CONSUMER(FA, DMX_PJ_WORDS6, DMX_PJ_RFL6, DMX_PJ_REST20)
              :
                [b0] "+v"(acc[0][1]),                [b1] "+v"(acc[1][1]),                [b2] "+v"(acc[2][1]),                [b3] "+v"(acc[3][1]),
                [b4] "+v"(acc[4][1]),                [b5] "+v"(acc[5][1]),                [b6] "+v"(acc[6][1]),                [b7] "+v"(acc[7][1]),
                [b8] "+v"(acc[8][1]),                [b9] "+v"(acc[9][1]),                [b10] "+v"(acc[10][1]),                [b11] "+v"(acc[11][1]),
                [b12] "+v"(acc[12][1]),                [b13] "+v"(acc[13][1]),                [b14] "+v"(acc[14][1]),                [b15] "+v"(acc[15][1]),
                [b16] "+v"(acc[16][1]),                [b17] "+v"(acc[17][1]),                [b18] "+v"(acc[18][1]),                [b19] "+v"(acc[19][1]),
                [b20] "+v"(acc[20][1]),                [b21] "+v"(acc[21][1]),                [b22] "+v"(acc[22][1]),                [b23] "+v"(acc[23][1]),
                [pj] "+v"(pj), [pi] "+v"(pi), [pt] "+v"(pt), [colv] "=&v"(colv),
                [t] "=&s"(tmp), [m0k] "=&s"(m0_keep), [ti] "=&s"(ti_c),
                [wa0] "=&s"(wa0), [wa1] "=&s"(wa1), [wa2] "=&s"(wa2), [wa3] "=&s"(wa3), [wa4] "=&s"(wa4), [wa5] "=&s"(wa5),
                [wb0] "=&s"(wb0), [wb1] "=&s"(wb1), [wb2] "=&s"(wb2), [wb3] "=&s"(wb3), [wb4] "=&s"(wb4), [wb5] "=&s"(wb5)
              : [tp] "s"(tp)
              : DMX_PJ_CLOB);
          } else {
            asm volatile(DMX_PJ_CONSUMER(ST, DMX_PJ_WORDS6, DMX_PJ_RFL6, DMX_PJ_REST20)
              :
                [a0] "+v"(acc[0][0]), [b0] "+v"(acc[0][1]),                [a1] "+v"(acc[1][0]), [b1] "+v"(acc[1][1]),
                [a2] "+v"(acc[2][0]), [b2] "+v"(acc[2][1]),                [a3] "+v"(acc[3][0]), [b3] "+v"(acc[3][1]),
                [a4] "+v"(acc[4][0]), [b4] "+v"(acc[4][1]),                [a5] "+v"(acc[5][0]), [b5] "+v"(acc[5][1]),
                [a6] "+v"(acc[6][0]), [b6] "+v"(acc[6][1]),                [a7] "+v"(acc[7][0]), [b7] "+v"(acc[7][1]),
                [a8] "+v"(acc[8][0]), [b8] "+v"(acc[8][1]),                [a9] "+v"(acc[9][0]), [b9] "+v"(acc[9][1]),
                [a10] "+v"(acc[10][0]), [b10] "+v"(acc[10][1]),                [a11] "+v"(acc[11][0]), [b11] "+v"(acc[11][1]),
                [a12] "+v"(acc[12][0]), [b12] "+v"(acc[12][1]),                [a13] "+v"(acc[13][0]), [b13] "+v"(acc[13][1]),
                [a14] "+v"(acc[14][0]), [b14] "+v"(acc[14][1]),                [a15] "+v"(acc[15][0]), [b15] "+v"(acc[15][1]),
                [a16] "+v"(acc[16][0]), [b16] "+v"(acc[16][1]),                [a17] "+v"(acc[17][0]), [b17] "+v"(acc[17][1]),
                [a18] "+v"(acc[18][0]), [b18] "+v"(acc[18][1]),                [a19] "+v"(acc[19][0]), [b19] "+v"(acc[19][1]),
                [a20] "+v"(acc[20][0]), [b20] "+v"(acc[20][1]),                [a21] "+v"(acc[21][0]), [b21] "+v"(acc[21][1]),
                [a22] "+v"(acc[22][0]), [b22] "+v"(acc[22][1]),                [a23] "+v"(acc[23][0]), [b23] "+v"(acc[23][1]),
                [pj] "+v"(pj), [pi] "+v"(pi), [pt] "+v"(pt), [colv] "=&v"(colv),
                [t] "=&s"(tmp), [m0k] "=&s"(m0_keep), [ti] "=&s"(ti_c),
                [wa0] "=&s"(wa0), [wa1] "=&s"(wa1), [wa2] "=&s"(wa2), [wa3] "=&s"(wa3), [wa4] "=&s"(wa4), [wa5] "=&s"(wa5),
                [wb0] "=&s"(wb0), [wb1] "=&s"(wb1), [wb2] "=&s"(wb2), [wb3] "=&s"(wb3), [wb4] "=&s"(wb4), [wb5] "=&s"(wb5)
              : [tp] "s"(tp)
              : DMX_PJ_CLOB);
          }
        } else {
          if constexpr (FAST) {
            asm volatile(DMX_PJ_CONSUMER(FA, DMX_PJ_WORDS5, DMX_PJ_RFL5, DMX_PJ_REST16)
              :
                [b0] "+v"(acc[0][1]),                [b1] "+v"(acc[1][1]),                [b2] "+v"(acc[2][1]),                [b3] "+v"(acc[3][1]),
                [b4] "+v"(acc[4][1]),                [b5] "+v"(acc[5][1]),                [b6] "+v"(acc[6][1]),                [b7] "+v"(acc[7][1]),
                [b8] "+v"(acc[8][1]),                [b9] "+v"(acc[9][1]),                [b10] "+v"(acc[10][1]),                [b11] "+v"(acc[11][1]),
                [b12] "+v"(acc[12][1]),                [b13] "+v"(acc[13][1]),                [b14] "+v"(acc[14][1]),                [b15] "+v"(acc[15][1]),
                [b16] "+v"(acc[16][1]),                [b17] "+v"(acc[17][1]),                [b18] "+v"(acc[18][1]),                [b19] "+v"(acc[19][1]),
                [pj] "+v"(pj), [pi] "+v"(pi), [pt] "+v"(pt), [colv] "=&v"(colv),
                [t] "=&s"(tmp), [m0k] "=&s"(m0_keep), [ti] "=&s"(ti_c),
                [wa0] "=&s"(wa0), [wa1] "=&s"(wa1), [wa2] "=&s"(wa2), [wa3] "=&s"(wa3), [wa4] "=&s"(wa4),
                [wb0] "=&s"(wb0), [wb1] "=&s"(wb1), [wb2] "=&s"(wb2), [wb3] "=&s"(wb3), [wb4] "=&s"(wb4)
              : [tp] "s"(tp)
              : DMX_PJ_CLOB);
          } else {
            asm volatile(DMX_PJ_CONSUMER(ST, DMX_PJ_WORDS5, DMX_PJ_RFL5, DMX_PJ_REST16)
              :
                [a0] "+v"(acc[0][0]), [b0] "+v"(acc[0][1]),                [a1] "+v"(acc[1][0]), [b1] "+v"(acc[1][1]),
                [a2] "+v"(acc[2][0]), [b2] "+v"(acc[2][1]),                [a3] "+v"(acc[3][0]), [b3] "+v"(acc[3][1]),
                [a4] "+v"(acc[4][0]), [b4] "+v"(acc[4][1]),                [a5] "+v"(acc[5][0]), [b5] "+v"(acc[5][1]),
                [a6] "+v"(acc[6][0]), [b6] "+v"(acc[6][1]),                [a7] "+v"(acc[7][0]), [b7] "+v"(acc[7][1]),
                [a8] "+v"(acc[8][0]), [b8] "+v"(acc[8][1]),                [a9] "+v"(acc[9][0]), [b9] "+v"(acc[9][1]),
                [a10] "+v"(acc[10][0]), [b10] "+v"(acc[10][1]),                [a11] "+v"(acc[11][0]), [b11] "+v"(acc[11][1]),
                [a12] "+v"(acc[12][0]), [b12] "+v"(acc[12][1]),                [a13] "+v"(acc[13][0]), [b13] "+v"(acc[13][1]),
                [a14] "+v"(acc[14][0]), [b14] "+v"(acc[14][1]),                [a15] "+v"(acc[15][0]), [b15] "+v"(acc[15][1]),
                [a16] "+v"(acc[16][0]), [b16] "+v"(acc[16][1]),                [a17] "+v"(acc[17][0]), [b17] "+v"(acc[17][1]),
                [a18] "+v"(acc[18][0]), [b18] "+v"(acc[18][1]),                [a19] "+v"(acc[19][0]), [b19] "+v"(acc[19][1]),
                [pj] "+v"(pj), [pi] "+v"(pi), [pt] "+v"(pt), [colv] "=&v"(colv),
                [t] "=&s"(tmp), [m0k] "=&s"(m0_keep), [ti] "=&s"(ti_c),
                [wa0] "=&s"(wa0), [wa1] "=&s"(wa1), [wa2] "=&s"(wa2), [wa3] "=&s"(wa3), [wa4] "=&s"(wa4),
                [wb0] "=&s"(wb0), [wb1] "=&s"(wb1), [wb2] "=&s"(wb2), [wb3] "=&s"(wb3), [wb4] "=&s"(wb4)
              : [tp] "s"(tp)
              : DMX_PJ_CLOB);
          }
        }
      }
      __syncthreads();
      if constexpr (FAST) {
        if (tbase + TP < np) phase1b_fast(tbase + TP, b ^ 1, ok);
        __syncthreads();
      }
    }
    if constexpr (FAST) {
      __syncthreads();                             // the producer's singlet column is in s_pG now
      if (!ok) flag_cell(flagged, cell);
    }
    if (owner) {
#pragma unroll
      for (int jj = 0; jj < NJM; ++jj) {
        const int jx = j0 + jj;
        if (jj < nj && jx < V) {
          double* o = grid + (((size_t)cell * V + jx) * V + lane) * A;
          o[0] = FAST ? s_pG[jx] : acc[jj][0]; o[1] = acc[jj][1];
        }
      }
    }
  }
#undef DMX_PJ_C0_SX
#undef DMX_PJ_C1_SX
#undef DMX_PJ_C0_SY
#undef DMX_PJ_C1_SY
#undef DMX_PJ_ADDS_ST
#undef DMX_PJ_ADDS_FA
#undef DMX_PJ_WORD4
#undef DMX_PJ_COLADDR_ST
#undef DMX_PJ_COLADDR_FA
#undef DMX_PJ_READS_ST_SX
#undef DMX_PJ_READS_ST_SY
#undef DMX_PJ_READS_FA_SX
#undef DMX_PJ_READS_FA_SY
#undef DMX_PJ_FIRST4
#undef DMX_PJ_REST16
#undef DMX_PJ_MID
#undef DMX_PJ_WORDS5
#undef DMX_PJ_WORDS6
#undef DMX_PJ_RFL6
#undef DMX_PJ_REST20
#undef DMX_PJ_CONSUMER
#undef DMX_PJ_RFL5
#undef DMX_PJ_NEXT
#undef DMX_PJ_END
#undef DMX_PJ_CLOB
}

// K2 over genotype classes, FAST mode, alpha grid {0, 0.5}: k_doublet_sym's entry set (singlet column + one evaluation per
// unordered pair) with k_doublet_cls's class table.  ONE WAVEFRONT PER BARCODE (four independent barcodes per workgroup, no
// workgroup barrier after the table staging): lane (j, q) owns NED consecutive rotation offsets d = q*NED .. q*NED+NED-1 of
// sample j, i.e. the pairs {j, (j+d) mod V}; lanes q = 0 also own the singlet entry [j][0][0].  Per tile of 32 pairs:
//   stage    headers, class rows (4 x 3 float32) and the pairs' 2-bit class ids as a stream over the periodic sample sequence
//            0..V-1,0..V-1,... (built once per SNP by k_build_classes) so that a lane's consecutive (j+d) mod V never wrap
//   phase 1  the five distinct pG values of alpha 0.5 and the three of alpha 0 (k_doublet_sym), the llks00 terms
//   per sub-tile of 8 pairs:
//   phase 1b T[pair][cj][ck] = log(row_cj . (pG[1] row_ck)) for cj <= ck (mirrored), T[pair][cj][4] = log(row_cj . (pG[0] row_c0)),
//            c0 = class of sample 0; 64-byte rows: a pair's table occupies the 64 LDS banks exactly once (conflict-free lookups)
//   phase 2  per pair and lane: its id window (2-4 words), then per entry one bit-field extract, one address op, one 8-byte LDS
//            lookup and one FP64 add.
template <int NED, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void k_doublet_clsym(PileupView pv, int nrd_width, const float* __restrict__ rows,
                                                               const uint32_t* __restrict__ idd, int32_t nwd2,
                                                               const double* __restrict__ gp0, const double* __restrict__ tabs,
                                                               const int32_t* __restrict__ sched, int32_t V,
                                                               double* __restrict__ grid, double* __restrict__ l00,
                                                               uint8_t* __restrict__ flagged) {
  constexpr int A = 2, TP = 32, TPC = 64, SUBT = 8;
  constexpr int CPW = kThreads / TPC;
  constexpr int T00 = TP + 2;
  constexpr int NW = 10;                          // id-stream words per pair (V <= 64: nwd2 <= 10)
  constexpr int NRW = (2 * NED + 30) / 32 + 1;    // words a lane's window can span
  constexpr int NT = 32;                          // class-table doubles per pair: [cj][8]: ck = 0..3 | singlet | pad
  extern __shared__ __attribute__((aligned(64))) unsigned char s_raw[];
  __shared__ double s_tab[kTab2];
  __shared__ double s_w[2][10];                  // mixing weights per alpha and distinct value (see k_doublet_sym)
  const double* s_log = s_tab + kLut2;
  const int t = threadIdx.x;
  stage_k2_tables(s_tab, tabs, t, kThreads);
  if (t < 10) {
    const int n = t / 5, q = t % 5;
    const int l = n ? (q > 2 ? 2 : q) : min(q, 2), m = n ? q - l : 0;
    const double p = 0.5 * l + (m - l) * 0.5 * (n ? 0.5 : 0.0);
    s_w[n][q] = p;
    s_w[n][5 + q] = 1.0 - p;
  }
  __syncthreads();

  const int cw = t / TPC, tid = t % TPC;
  constexpr size_t cell_bytes = ((size_t)SUBT * NT * 8 + (size_t)TP * 6 * 8 + (size_t)TP * 4 * 8 + 2 * T00 * 8 + TP * (4 + 4 + 8) +
                                 (size_t)TP * 12 * 4 + (size_t)TP * NW * 4 + 63) & ~(size_t)63;
  unsigned char* base = s_raw + (size_t)cw * cell_bytes;
  double* s_T = (double*)base;                                   // [SUBT][4][8]  (a pair's 256 contiguous bytes = each of the 64 banks once)
  double* s_q1 = s_T + SUBT * NT;                                // [TP][6]   pG of alpha 0.5: q[l+m]
  double* s_q0 = s_q1 + TP * 6;                                  // [TP][4]   pG of alpha 0:   q[l]
  double* s_t00 = s_q0 + TP * 4;                                 // [2][T00]
  int64_t* s_off = (int64_t*)(s_t00 + 2 * T00);                  // [TP]
  int32_t* s_snp = (int32_t*)(s_off + TP);                       // [TP]
  uint32_t* s_cnt = (uint32_t*)(s_snp + TP);                     // [TP]
  float* s_rows = (float*)(s_cnt + TP);                          // [TP][4][3]
  uint32_t* s_pk = (uint32_t*)(s_rows + TP * 12);                // [TP][NW]  2-bit ids of samples 0..V-1,0..V-1,...

  const int slot = blockIdx.x * CPW + cw;
  if (slot >= pv.B) return;                      // whole wavefront idle (no workgroup barriers below)
  const int32_t cell = sched[slot];
  const int64_t p_beg = pv.cell_pair_off[cell];
  const int64_t np = pv.cell_pair_off[cell + 1] - p_beg;
  int64_t rd_base = pv.cell_read_off[cell];

  // phase-2 identity
  const int D = V / 2 + 1;                        // rotation offsets 0..V/2
  // Panels whose D offsets do not fit one wavefront's (64 / V) x NED are cut into slabs of offsets, one wavefront (blockIdx.y)
  // each, which repeat the cheap phases 1 and 1b for themselves: no barrier, and more, shorter wavefronts per barcode.
  const int j = tid % V, q = tid / V;
  const int d0 = ((int)blockIdx.y * (TPC / V) + q) * NED;
  const bool lane_on = d0 < D && q * V + V <= TPC;   // the lane owns at least one offset (and is a complete (j,q) row)
  const int p0 = lane_on ? j + d0 : 0;            // first position of its window in the id stream
  const uint32_t w0 = (uint32_t)p0 >> 4, sh0 = ((uint32_t)p0 & 15u) * 2u;
  const uint32_t wj = (uint32_t)j >> 4, shj = ((uint32_t)j & 15u) * 2u;
  const bool sing_owner = tid < V && blockIdx.y == 0;   // lanes q = 0 of the first slab
  double acc[NED], accS = 0.0;
#pragma unroll
  for (int i = 0; i < NED; ++i) acc[i] = 0.0;
  bool ok = true;
  const int ti1 = tid >> 1, n1 = tid & 1;
  double acc00 = 0.0;

  // The two-wavefront-per-SIMD forms (one slab of up to 33 offsets) have registers to spare and little else to hide memory
  // latency with: they run a two-deep pipeline like K1's.  While tile t computes, the header of tile t + 2 and everything tile
  // t + 1 reads from global memory (class rows, id streams, leading read bytes, gp0) are in flight into registers.
  constexpr bool PF = MINW <= 2;
  constexpr int NR_ROWS = TP * 12 / TPC, NR_PK = TP * NW / TPC;   // per-lane registers of a tile's rows (6) and id words (5)
  uint32_t hd_n = 0u; int32_t hd_s = 0;          // header (stored reads, SNP id) of this lane's pair in the NEXT tile (PF: tile + 2)
  uint32_t pn = 0u; int32_t psn = 0; int64_t poff = 0;             // PF: prepared header of the tile whose data is in flight
  float d_rows[NR_ROWS]; uint32_t d_pk[NR_PK]; uint32_t d_rd4 = 0u; double d_g0[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < NR_ROWS; ++i) d_rows[i] = 0.f;
#pragma unroll
  for (int i = 0; i < NR_PK; ++i) d_pk[i] = 0u;
  auto load_hdr = [&](int64_t first) {           // header loads of the tile that starts at pair `first`
    hd_n = 0u; hd_s = 0;
    const int64_t nx = first + tid;
    if (tid < TP && nx < np) { hd_n = load_nrd(pv.pair_nrd, p_beg + nx, nrd_width); hd_s = pv.pair_snp ? pv.pair_snp[p_beg + nx] : (int32_t)nx; }
  };
  auto prepare = [&]() {                         // PF: hd_* (arrived) -> pn/psn/poff, then request that tile's data
    pn = hd_n; psn = hd_s;
    const uint32_t incl = seg_scan_incl<32>(pn);
    poff = rd_base + (int64_t)(incl - pn);
    rd_base += (int64_t)__shfl(incl, 31);        // lanes >= 32 carry zeros: lane 31 holds the tile's read count
#pragma unroll
    for (int i = 0; i < NR_ROWS; ++i) {
      const int e = tid + TPC * i;
      d_rows[i] = rows[(size_t)__shfl(psn, e / 12) * 12 + (e % 12)];
    }
#pragma unroll
    for (int i = 0; i < NR_PK; ++i) {
      const int e = tid + TPC * i, w = e % NW;
      const int32_t sn_e = __shfl(psn, e / NW);
      d_pk[i] = w < nwd2 ? idd[(size_t)sn_e * nwd2 + w] : 0u;
    }
    const uint32_t cnt1 = __shfl(pn, ti1);
    const int64_t off1 = ((int64_t)__shfl((int)(poff >> 32), ti1) << 32) | (uint32_t)__shfl((int)(uint32_t)poff, ti1);
    d_rd4 = load_rd4(pv, off1, cnt1);
    const double* g0 = gp0 + (size_t)__shfl(psn, ti1) * 3;
    d_g0[0] = g0[0]; d_g0[1] = g0[1]; d_g0[2] = g0[2];
  };
  load_hdr(0);
  if (PF) { prepare(); load_hdr(TP); }
  for (int64_t tbase = 0; tbase < np; tbase += TP) {
    const int tp = (int)min((int64_t)TP, np - tbase);
    uint32_t rd4_cur = 0u; double g0_cur[3] = {0.0, 0.0, 0.0};
    if (PF) {
      // this tile's data (requested a tile ago) -> LDS; then prepare the next tile and request the one after's header
      if (tid < TP) { s_cnt[tid] = pn; s_off[tid] = poff; s_snp[tid] = psn; }
#pragma unroll
      for (int i = 0; i < NR_ROWS; ++i) s_rows[tid + TPC * i] = d_rows[i];
#pragma unroll
      for (int i = 0; i < NR_PK; ++i) s_pk[tid + TPC * i] = d_pk[i];
      rd4_cur = d_rd4; g0_cur[0] = d_g0[0]; g0_cur[1] = d_g0[1]; g0_cur[2] = d_g0[2];
      prepare();
      load_hdr(tbase + 2 * TP);
      DMX_WAVE_LDS_ORDER();
    } else {
    if (tid < TP) {
      const uint32_t n = hd_n;                     // this tile's header was requested a tile ago; now request the next one's
      const int32_t sn = hd_s;
      const int64_t nx = tbase + TP + tid;
      hd_n = 0u; hd_s = 0;
      if (nx < np) { hd_n = load_nrd(pv.pair_nrd, p_beg + nx, nrd_width); hd_s = pv.pair_snp ? pv.pair_snp[p_beg + nx] : (int32_t)nx; }
      publish_tile_headers<TP>(n, sn, tid, rd_base, s_cnt, s_off, s_snp);
    }
    DMX_WAVE_LDS_ORDER();
    rd_base = s_off[tp - 1] + (int64_t)s_cnt[tp - 1];
    // ---- class rows and id streams -> LDS
    for (int e = tid; e < tp * 12; e += TPC) s_rows[e] = rows[(size_t)s_snp[e / 12] * 12 + (e % 12)];
    for (int e = tid; e < tp * NW; e += TPC) {
      const int ti = e / NW, w = e % NW;
      s_pk[e] = w < nwd2 ? idd[(size_t)s_snp[ti] * nwd2 + w] : 0u;
    }
    }
    // ---- phase 1 (five distinct values per alpha lane)
    {
      const bool on = ti1 < tp;
      const uint32_t cnt = on ? s_cnt[ti1] : 0u;
      const int64_t off = on ? s_off[ti1] : 0;
      const uint32_t rd4 = PF ? rd4_cur : load_rd4(pv, off, cnt);   // the first four read bytes in one load (one dependent latency instead of four)
      const int32_t snp1 = on ? s_snp[ti1] : 0;
      double qv[5], wA[5], wR[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) { wA[i] = s_w[n1][i]; wR[i] = s_w[n1][5 + i]; }
      const double mx = pair_values_open<5>(pv, cnt, off, rd4, s_tab, wA, wR, n1, qv);
      if (on) {
        const double y = rcp_refined(mx);
#pragma unroll
        for (int i = 0; i < 5; ++i) qv[i] = div_by(qv[i], mx, y);            // :656-663
        const double* g0 = gp0 + (size_t)snp1 * 3;
        const double qq[3] = {PF ? g0_cur[0] : g0[0], PF ? g0_cur[1] : g0[1], PF ? g0_cur[2] : g0[2]};
        double sum = 0.0;
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            const double v = n1 ? qv[l + m] : qv[l];                         // pG[n][l][m] (not llks00_term: see k_doublet_sym)
            sum += ((qq[l] * qq[m]) * v);                                    // :555, :702-705
          }
        ok &= __builtin_amdgcn_class(sum, 0x100);
        s_t00[n1 * T00 + ti1] = dmx_log2_fast(sum, s_log);
        if (n1) {
#pragma unroll
          for (int i = 0; i < 5; ++i) s_q1[ti1 * 6 + i] = qv[i];
        } else {
#pragma unroll
          for (int i = 0; i < 3; ++i) s_q0[ti1 * 4 + i] = qv[i];
        }
      }
    }
    DMX_WAVE_LDS_ORDER();
    if (tid < 2) {
      const double* row = &s_t00[tid * T00];
      if (tp == TP) {                              // eight terms at a time: loads first, then the ordered adds
#pragma unroll 1
        for (int h = 0; h < TP; h += 8) {
          double2 v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const double2*>(&row[h + 2 * i]);
#pragma unroll
          for (int i = 0; i < 4; ++i) { acc00 += v[i].x; acc00 += v[i].y; }
        }
      } else {
        for (int i = 0; i < tp; ++i) acc00 += row[i];
      }
    }
#pragma unroll 1
    for (int sub = 0; sub < tp; sub += SUBT) {
      const int ns = min(SUBT, tp - sub);
      // ---- phase 1b: the class table of the sub-tile's pairs (bilinear form row_cj . (pG row_ck)); 14 items per pair:
      //      ten unordered class pairs cj <= ck (stored to both [cj][ck] and [ck][cj]) and the four singlet entries
      for (int e = tid; e < ns * 14; e += TPC) {
        const int pi = e / 14, c = e % 14;
        const int ti = sub + pi;
        const int cj = c < 10 ? (int)((0x3221110000ull >> (4 * c)) & 15u) : c - 10;        // (0,0)(0,1)(0,2)(0,3)(1,1)(1,2)(1,3)(2,2)(2,3)(3,3)
        const int ck = c < 10 ? (int)((0x3323213210ull >> (4 * c)) & 15u) : (int)(s_pk[ti * NW] & 3u);   // singlet: sample 0's class
        const float* rj = &s_rows[ti * 12 + cj * 3];
        const float* rk = &s_rows[ti * 12 + ck * 3];
        const double a0 = (double)rj[0], a1 = (double)rj[1], a2 = (double)rj[2];
        const double b0 = (double)rk[0], b1 = (double)rk[1], b2 = (double)rk[2];
        double u0, u1, u2;
        if (c < 10) {
          const double* P = &s_q1[ti * 6];                                   // pG[1][l][m] = P[l + m]
          u0 = __builtin_fma(P[2], b2, __builtin_fma(P[1], b1, P[0] * b0));
          u1 = __builtin_fma(P[3], b2, __builtin_fma(P[2], b1, P[1] * b0));
          u2 = __builtin_fma(P[4], b2, __builtin_fma(P[3], b1, P[2] * b0));
        } else {
          const double* P = &s_q0[ti * 4];                                   // pG[0][l][m] = P[l]
          u0 = __builtin_fma(P[0], b2, __builtin_fma(P[0], b1, P[0] * b0));
          u1 = __builtin_fma(P[1], b2, __builtin_fma(P[1], b1, P[1] * b0));
          u2 = __builtin_fma(P[2], b2, __builtin_fma(P[2], b1, P[2] * b0));
        }
        const double sum = __builtin_fma(a2, u2, __builtin_fma(a1, u1, a0 * u0));
        ok &= __builtin_amdgcn_class(sum, 0x100);
        const double lv = dmx_log2_fast(sum, s_log);
        if (c < 10) { s_T[pi * NT + cj * 8 + ck] = lv; s_T[pi * NT + ck * 8 + cj] = lv; }
        else s_T[pi * NT + cj * 8 + 4] = lv;
      }
      DMX_WAVE_LDS_ORDER();
      // ---- phase 2.  LDS byte address of an entry's table cell = (row base of this pair and this lane's class cj, a multiple of
      //      64) | (ck << 3): one shift and one and-or per entry.  Entries go in groups of GRP (their loads in flight together).
      if (lane_on) {
#ifdef DMX_CLSYM_GRP
        constexpr int GRP = NED <= DMX_CLSYM_GRP ? NED : (NED + (NED + DMX_CLSYM_GRP - 1) / DMX_CLSYM_GRP - 1) / ((NED + DMX_CLSYM_GRP - 1) / DMX_CLSYM_GRP);   // kernel experiments only
#else
        constexpr int GRP = NED <= 12 ? NED : (NED + 2) / 3;
#endif
        using lds_cd = const __attribute__((address_space(3))) double*;
        using lds_cu = const __attribute__((address_space(3))) uint32_t*;
        const uint32_t t_base = (uint32_t)(uintptr_t)(lds_cd)s_T;            // 64-byte aligned (checked by the launcher's layout)
        const uint32_t pk_lane = (uint32_t)(uintptr_t)(lds_cu)s_pk + 4u * w0, pk_j = (uint32_t)(uintptr_t)(lds_cu)s_pk + 4u * wj;
#ifdef DMX_CLSYM_UNR
        constexpr int UNR = DMX_CLSYM_UNR;             // kernel experiments only
#else
        constexpr int UNR = NED >= 12 ? 1 : 2;
#endif
#pragma unroll UNR
        for (int pi = 0; pi < ns; ++pi) {
          const uint32_t po = (uint32_t)((sub + pi) * NW * 4);
          const uint32_t cj = (*(lds_cu)(uintptr_t)(pk_j + po) >> shj) & 3u;
          uint32_t wd[NRW];
#pragma unroll
          for (int r = 0; r < NRW; ++r) wd[r] = *(lds_cu)(uintptr_t)(pk_lane + po + 4u * r);
          const uint32_t row = t_base + (uint32_t)(pi * NT * 8) + (cj << 6);
          uint32_t bits[(NED + 15) / 16];
#pragma unroll
          for (int r = 0; r < (NED + 15) / 16; ++r)     // ids of (j + d0 + i) mod V: 16 per funnel-shifted word
            bits[r] = (r + 1 < NRW) ? __builtin_amdgcn_alignbit(wd[r + 1], wd[r], sh0) : (wd[r] >> sh0);
#pragma unroll
          for (int g0 = 0; g0 < NED; g0 += GRP) {
            double tv[GRP];
#pragma unroll
            for (int i = g0; i < g0 + GRP && i < NED; ++i) {
              const int sh = 2 * (i % 16) - 3;           // ck << 3
              const uint32_t b = bits[i / 16];
              const uint32_t a = row | ((sh >= 0 ? (b >> sh) : (b << -sh)) & 24u);
              tv[i - g0] = *(lds_cd)(uintptr_t)a;
            }
#pragma unroll
            for (int i = g0; i < g0 + GRP && i < NED; ++i) acc[i] += tv[i - g0];
            if (g0 + GRP < NED) __builtin_amdgcn_sched_barrier(0);
          }
          if (sing_owner) accS += *(lds_cd)(uintptr_t)(row + 32u);
        }
      }
      DMX_WAVE_LDS_ORDER();
    }
  }
  {
    double* G = grid + (size_t)cell * V * V * A;
    if (lane_on) {
#pragma unroll
      for (int i = 0; i < NED; ++i) {
        const int d = d0 + i;
        if (d < D) {
          int k = j + d; k = k >= V ? k - V : k;
          if (!(2 * d == V && j > k)) {            // d = V/2 is reached from both sides: the j < k lane stores
            G[((size_t)j * V + k) * A + 1] = acc[i];
            G[((size_t)k * V + j) * A + 1] = acc[i];
          }
        }
      }
      if (sing_owner) for (int k = 0; k < V; ++k) G[((size_t)j * V + k) * A] = accS;
    }
    if (tid < 2 && blockIdx.y == 0) l00[(size_t)cell * A + tid] = acc00;
    if (!ok) flag_cell(flagged, cell);
  }
}

// K2 over genotype classes for alpha grids of 3..8 entries: k_doublet_cls with k_doublet_an's phase 1.  The class table holds
// T[pair][cj][ck][n] for the AP padded alphas; phase 2 is AP/2 16-byte lookups and A adds per (j, k).
template <int TPC, int NK, int AP>
__global__ __launch_bounds__(kThreads) void k_doublet_clsn(PileupView pv, int nrd_width, const float* __restrict__ rows,
                                                           const uint8_t* __restrict__ ids, const double* __restrict__ gp0,
                                                           const double* __restrict__ tabs, const double* __restrict__ alpha,
                                                           const int32_t* __restrict__ sched, int32_t V, int32_t A, int32_t VS,
                                                           double* __restrict__ grid, double* __restrict__ l00,
                                                           uint8_t* __restrict__ flagged) {
  static_assert(AP == 4 || AP == 8, "alphas per pair padded to a power of two");
  constexpr int TP = 32;
  constexpr int CPW = kThreads / TPC;
  constexpr int T00 = TP + 2;
  constexpr int NT = kMaxCls * kMaxCls * AP;     // class-table entries per pair
#define DMX_K2_SYNC() do { if (TPC == 64) { DMX_WAVE_LDS_ORDER(); } else { __syncthreads(); } } while (0)
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_tab[kTab2];
  const double* s_log = s_tab + kLut2;
  const int t = threadIdx.x;
  stage_k2_tables(s_tab, tabs, t, kThreads);
  __syncthreads();

  const int cw = t / TPC, tid = t % TPC;
  const size_t cell_bytes = (size_t)TP * AP * 9 * 8 + (size_t)TP * NT * 8 + (size_t)AP * T00 * 8 + TP * (4 + 4 + 8) + (size_t)TP * 12 * 4 + (size_t)TP * VS;
  unsigned char* base = s_raw + (size_t)cw * ((cell_bytes + 15) & ~(size_t)15);
  double* s_pG = (double*)base;                                  // [TP][AP][9]
  double* s_T = s_pG + TP * AP * 9;                              // [TP][4][4][AP]
  double* s_t00 = s_T + TP * NT;                                 // [AP][T00]
  int64_t* s_off = (int64_t*)(s_t00 + AP * T00);                 // [TP]
  int32_t* s_snp = (int32_t*)(s_off + TP);                       // [TP]
  uint32_t* s_cnt = (uint32_t*)(s_snp + TP);                     // [TP]
  float* s_rows = (float*)(s_cnt + TP);                          // [TP][4][3]
  uint8_t* s_ids = (uint8_t*)(s_rows + TP * 12);                 // [TP][VS]

  const int slot = blockIdx.x * CPW + cw;
  if (TPC == 64 && slot >= pv.B) return;
  const bool cell_ok = slot < pv.B;
  const int32_t cell = cell_ok ? sched[slot] : 0;
  const int64_t p_beg = cell_ok ? pv.cell_pair_off[cell] : 0;
  const int64_t np = cell_ok ? pv.cell_pair_off[cell + 1] - p_beg : 0;
  int64_t rd_base = cell_ok ? pv.cell_read_off[cell] : 0;

  const int KB = (V + NK - 1) / NK;
  const int JS = TPC / KB;
  const int jl = tid / KB, kb = tid % KB;
  const int j = (int)blockIdx.y * JS + jl;
  const bool owner = jl < JS && j < V;
  double acc[NK][AP];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk)
#pragma unroll
    for (int n = 0; n < AP; ++n) acc[kk][n] = 0.0;
  bool ok = true;
  double acc00 = 0.0;
  constexpr int P1 = TP * AP;                    // phase-1 lanes per tile
  constexpr int NPASS = (P1 + TPC - 1) / TPC;
  const int n1 = tid % AP;                       // this thread's alpha in phase 1 (TPC is a multiple of AP)
  const bool n_ok = n1 < A;
  double wA[9], wR[9];
  {
    const double al = n_ok ? alpha[n1] : 0.0;
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const double p = 0.5 * l + (m - l) * 0.5 * al;                       // :613
        wA[l * 3 + m] = p;
        wR[l * 3 + m] = 1.0 - p;
      }
  }


  for (int64_t tbase = 0; tbase < np; tbase += TP) {
    const int tp = (int)min((int64_t)TP, np - tbase);
    load_tile_headers<TP>(pv, nrd_width, p_beg, tbase, tp, tid, rd_base, s_cnt, s_off, s_snp);
    DMX_K2_SYNC();
    rd_base = s_off[tp - 1] + (int64_t)s_cnt[tp - 1];
    for (int e = tid; e < tp * 12; e += TPC) s_rows[e] = rows[(size_t)s_snp[e / 12] * 12 + (e % 12)];
    {
      const int wpr = VS / 4;
      for (int e = tid; e < tp * wpr; e += TPC) {
        const int ti = e / wpr, wq = e % wpr;
        const uint8_t* src = ids + (size_t)s_snp[ti] * V + wq * 4;
        uint32_t wv = 0;
        for (int b = 0; b < 4; ++b) if (wq * 4 + b < V) wv |= (uint32_t)src[b] << (8 * b);
        reinterpret_cast<uint32_t*>(s_ids)[ti * wpr + wq] = wv;
      }
    }
    // ---- phase 1: lane u = (pair u / AP, alpha u % AP)
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
      const int u = tid + pass * TPC;
      if (u >= P1) break;                          // uniform per wavefront (P1 and TPC are multiples of 64)
      const int ti1 = u / AP;
      const bool on = ti1 < tp && n_ok;
      const uint32_t cnt = (ti1 < tp) ? s_cnt[ti1] : 0u;
      const int64_t off = (ti1 < tp) ? s_off[ti1] : 0;
      double pG[9];
      const double mx = pair_values_open<9, AP, true, false>(pv, cnt, off, 0u, s_tab, wA, wR, n1, pG, nullptr, n_ok);
      if (on) {
        const double y = rcp_refined(mx);                                    // numerators >= 1e-6, mx in [1e-6, 1+1e-6]
        ok &= llks00_term(gp0, s_snp[ti1], [&](int l, int m) { const double v = div_by(pG[l * 3 + m], mx, y); s_pG[(ti1 * AP + n1) * 9 + l * 3 + m] = v; return v; },
                    s_log, &s_t00[n1 * T00 + ti1]);                      // :656-663 into the llks00 term
      }
    }
    DMX_K2_SYNC();
    if (tid < A) {                                 // llks00[n]: lane n adds its alpha's terms in pair order
      const double* row = &s_t00[tid * T00];
      for (int i = 0; i < tp; ++i) acc00 += row[i];
    }
    // ---- phase 1b: the class table (padding alphas are skipped; their slots are never read)
    for (int e = tid; e < tp * NT; e += TPC) {
      const int ti = e / NT, cc = e % NT;
      const int n = cc % AP, ck = (cc / AP) & 3, cj = cc / (AP * 4);
      if (n >= A) continue;
      const float* rj = &s_rows[ti * 12 + cj * 3];
      const float* rk = &s_rows[ti * 12 + ck * 3];
      const double* P = &s_pG[(ti * AP + n) * 9];
      const double aj[3] = {(double)rj[0], (double)rj[1], (double)rj[2]};
      const double bk[3] = {(double)rk[0], (double)rk[1], (double)rk[2]};
      double sum = 0.0;                                                          // :674
#pragma unroll
      for (int l = 0; l < 3; ++l)
#pragma unroll
        for (int m = 0; m < 3; ++m) sum += ((aj[l] * bk[m]) * P[l * 3 + m]);     // :553, :677-679
      ok &= __builtin_amdgcn_class(sum, 0x100);
      s_T[ti * NT + cc] = dmx_log2_fast(sum, s_log);                              // the :683 term
    }
    DMX_K2_SYNC();
    // ---- phase 2
    if (owner) {
      for (int ti = 0; ti < tp; ++ti) {
        const uint8_t* idr = &s_ids[ti * VS];
        const int cj = idr[j];
        const double* Tj = &s_T[ti * NT + cj * 4 * AP];
#pragma unroll
        for (int kk = 0; kk < NK; ++kk) {
          const int k = min(kb * NK + kk, V - 1);
          const double* Tk = &Tj[idr[k] * AP];
#pragma unroll
          for (int h = 0; h < AP / 2; ++h) {
            if (2 * h >= A) break;
            const double2 tv = *reinterpret_cast<const double2*>(&Tk[2 * h]);
            acc[kk][2 * h] += tv.x;                                               // :683
            if (2 * h + 1 < A) acc[kk][2 * h + 1] += tv.y;
          }
        }
      }
    }
    DMX_K2_SYNC();
  }
  if (cell_ok) {
    if (owner) {
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        const int k = kb * NK + kk;
        if (k < V) {
          double* o = grid + (((size_t)cell * V + j) * V + k) * A;
#pragma unroll
          for (int n = 0; n < AP; ++n) if (n < A) o[n] = acc[kk][n];
        }
      }
    }
    if (tid < A && blockIdx.y == 0) l00[(size_t)cell * A + tid] = acc00;
    if (!ok) flag_cell(flagged, cell);
  }
#undef DMX_K2_SYNC
}

// Which genotype matrices can make a phase-2 log() argument leave the normal positive range at all?  Only those with a row that
// holds a NaN / infinity / negative entry or no entry above 2^-400 (see k_doublet_a2's CHK).  Sets *unsafe when it finds one.
__global__ void k_check_geno(const float* __restrict__ g, int64_t n_rows, int32_t* __restrict__ unsafe) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += (int64_t)gridDim.x * blockDim.x) {
    const float a = g[3 * i], b = g[3 * i + 1], c = g[3 * i + 2];
    const bool fin = (a >= 0.f) && (b >= 0.f) && (c >= 0.f) && (a <= 3.0e38f) && (b <= 3.0e38f) && (c <= 3.0e38f);   // false for NaN
    bad |= !fin || !(fmaxf(a, fmaxf(b, c)) >= 1e-30f);             // float32: anything normal is far above 2^-400
  }
  if (bad) atomicOr(unsafe, 1);
}

// ---------------------------------------------------------------------------------------------------------------------
// K3.  One cell per workgroup over its finished grid.
struct ArgMax { double v; int32_t i; };
__device__ __forceinline__ ArgMax better(ArgMax a, ArgMax b) {      // larger value wins; equal values: lower scan index
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

__global__ __launch_bounds__(kThreads) void k_reduce(const double* __restrict__ grid, const double* __restrict__ l00,
                                                     const int64_t* __restrict__ cell_pair_off,
                                                     const double* __restrict__ alpha, int32_t V, int32_t A,
                                                     double prior, dmx_cell_summary* __restrict__ out,
                                                     double* __restrict__ sing) {
  __shared__ double s_d[kThreads];
  __shared__ double s_e[kThreads];
  __shared__ int32_t s_i[kThreads];
  const int t = threadIdx.x;
  const int32_t cell = blockIdx.x;
  const int32_t nAB = V * V * A;
  const double* G = grid + (size_t)cell * nAB;
  const int32_t npairs = (int32_t)(cell_pair_off[cell + 1] - cell_pair_off[cell]);

  for (int32_t jj = t; jj < V; jj += kThreads) sing[(size_t)cell * V + jj] = G[(size_t)jj * V * A];   // llksAB[j][0][0]
  // (1) max over the whole grid (:713-721)
  double mx = -1e300;
  for (int32_t q = t; q < nAB; q += kThreads) mx = fmax(mx, G[q]);
  s_d[t] = mx;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) s_d[t] = (s_d[t] < s_d[t + s]) ? s_d[t + s] : s_d[t];
    __syncthreads();
  }
  const double max_llk = s_d[0];
  __syncthreads();

  // (2) posterior sums (:724-734) — same per-term expression, tree order for the sum
  double ss = 0.0, sd = 0.0;
  for (int32_t q = t; q < nAB; q += kThreads) {
    const int32_t n = q % A, jk = q / A, j = jk / V, k = jk % V;
    const double e = exp(G[q] - max_llk);
    if (k == 0 && n == 0) ss += (e * (1. - prior) / V);
    if (j != k && n >= 1) sd += (e * prior / V / (V - 1) / (A - 1) / (alpha[n] == 0.5 ? 2.0 : 1.0));
  }
  s_d[t] = ss; s_e[t] = sd;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) { s_d[t] += s_d[t + s]; s_e[t] += s_e[t + s]; }
    __syncthreads();
  }
  const double sum_single = s_d[0], sum_double = s_e[0];
  __syncthreads();

  // (3) best doublet: first maximum in (j,k,n) scan order over j != k, n >= 1 (:799-814)
  ArgMax bd{-1e300, 0x7FFFFFFF};
  for (int32_t q = t; q < nAB; q += kThreads) {
    const int32_t n = q % A, jk = q / A, j = jk / V, k = jk % V;
    if (j != k && n >= 1) bd = better(bd, ArgMax{G[q], q});
  }
  s_d[t] = bd.v; s_i[t] = bd.i;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) { ArgMax r = better(ArgMax{s_d[t], s_i[t]}, ArgMax{s_d[t + s], s_i[t + s]}); s_d[t] = r.v; s_i[t] = r.i; }
    __syncthreads();
  }
  const int32_t qbest = s_i[0];
  __syncthreads();

  // (4) top-2 singlets from llksAB[j][0][0] (:746-758)
  ArgMax b1{-1e300, 0x7FFFFFFF};
  for (int32_t j = t; j < V; j += kThreads) b1 = better(b1, ArgMax{G[(size_t)j * V * A], j});
  s_d[t] = b1.v; s_i[t] = b1.i;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) { ArgMax r = better(ArgMax{s_d[t], s_i[t]}, ArgMax{s_d[t + s], s_i[t + s]}); s_d[t] = r.v; s_i[t] = r.i; }
    __syncthreads();
  }
  const int32_t i1 = s_i[0];
  __syncthreads();
  ArgMax b2{-1e300, 0x7FFFFFFF};
  for (int32_t j = t; j < V; j += kThreads) if (j != i1) b2 = better(b2, ArgMax{G[(size_t)j * V * A], j});
  s_d[t] = b2.v; s_i[t] = b2.i;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) { ArgMax r = better(ArgMax{s_d[t], s_i[t]}, ArgMax{s_d[t + s], s_i[t + s]}); s_d[t] = r.v; s_i[t] = r.i; }
    __syncthreads();
  }
  const int32_t i2 = (s_i[0] == 0x7FFFFFFF) ? -1 : s_i[0];

  // (5) decisions within 1e-7 of an alternative (other than the alpha = 0.5 mirror of the best doublet, which every cell has):
  //     the host fetches the grid of such a cell and lets the tie arbiter re-evaluate the contenders (DESIGN.md "Ties")
  int32_t flags = 0;
  {
    const double tol = 1e-7;
    bool near_d = false;
    if (qbest != 0x7FFFFFFF) {
      const double best = G[qbest];
      const int32_t nb = qbest % A, jkb = qbest / A, jb = jkb / V, kb = jkb % V;
      const int32_t qmir = (alpha[nb] == 0.5) ? ((kb * V + jb) * A + nb) : -1;
      for (int32_t q = t; q < nAB; q += kThreads) {
        const int32_t n = q % A, jk = q / A, j = jk / V, k = jk % V;
        if (j != k && n >= 1 && q != qbest && q != qmir && G[q] >= best - tol) near_d = true;
      }
    }
    int cnt = 0;
    const double s1v = (i1 != 0x7FFFFFFF) ? G[(size_t)i1 * V * A] : 0.0, s2v = (i2 >= 0) ? G[(size_t)i2 * V * A] : -1e300;
    for (int32_t j = t; j < V; j += kThreads) if (G[(size_t)j * V * A] >= s2v - tol) ++cnt;
    const int any_d = __syncthreads_or(near_d ? 1 : 0);
    s_i[t] = cnt;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if (t < s) s_i[t] += s_i[t + s];
      __syncthreads();
    }
    const int n_near_s = s_i[0];
    if (any_d) flags |= DMX_CELL_NEAR_DOUBLET;
    if (i2 >= 0 && (n_near_s > 2 || s1v - s2v < tol)) flags |= DMX_CELL_NEAR_SINGLET;
  }

  if (t == 0) {
    // NaN likelihoods (e.g. a GP record with a missing sample poisons the whole SNP, bcf_filtered_reader.cpp:431-448) make
    // every `<` of the reference's scans false: it then indexes with -1 (:816-825, undefined behaviour).  Here the
    // indices stay -1 and the dependent values are NaN; nothing is read out of bounds.
    const double kNaN = __builtin_nan("");
    dmx_cell_summary r;
    r.max_llk = max_llk; r.sum_single = sum_single; r.sum_double = sum_double;
    const bool has1 = i1 != 0x7FFFFFFF, hasb = qbest != 0x7FFFFFFF;
    r.i_sing1 = has1 ? i1 : -1; r.i_sing2 = i2;
    r.sing_llk1 = has1 ? G[(size_t)i1 * V * A] : kNaN;
    r.sing_llk2 = (i2 >= 0) ? G[(size_t)i2 * V * A] : -1e300;
    const int32_t nb = hasb ? qbest % A : 0, jkb = hasb ? qbest / A : 0, jb = jkb / V, kb = jkb % V;
    r.j_best = hasb ? jb : -1; r.k_best = hasb ? kb : -1; r.n_best = hasb ? nb : -1;
    r.llk12 = hasb ? G[qbest] : kNaN;
    r.llk1 = hasb ? G[(size_t)jb * V * A] : kNaN; r.llk2 = hasb ? G[(size_t)kb * V * A] : kNaN;
    r.llk10 = hasb ? G[(size_t)jb * V * A + nb] : kNaN; r.llk20 = hasb ? G[(size_t)kb * V * A + nb] : kNaN;    // :824-825
    r.llk00_0 = l00[(size_t)cell * A]; r.llk00_best = l00[(size_t)cell * A + nb];
    // (6) the BEST rule's own comparisons (:837,:844) with a margin below 1e-7: the writers re-evaluate the entries involved (dmx::near_rule)
    if (hasb && has1 && i2 >= 0) {
      const double tol = 1e-7, s1 = r.sing_llk1, s2 = r.sing_llk2;
      if (fabs(r.llk12 - (s1 + 2)) < tol || fabs(s1 - (s2 + 2)) < tol ||
          ((fabs(r.llk12 - r.llk1) < tol || fabs(r.llk12 - r.llk2) < tol) && r.llk12 > s1 + 2 - tol))
        flags |= DMX_CELL_NEAR_RULE;
    }
    r.n_pairs = npairs; r.flags = flags; r.reserved = 0; r.llk_ab = 0.0; r.llk_ba = 0.0;
    r.llk_ab_alt = 0.0; r.llk_ba_alt = 0.0; r.ev_x_ab = 0.0; r.ev_t_ab = 0.0; r.ev_x_ba = 0.0; r.ev_t_ba = 0.0;
    out[cell] = r;
  }
}

// ---- anchored doublet search (dmx_engine_doublet_anchored) -----------------------------------------------------
// Entries of the grid llksAB[V][V][A] without the grid: column 0 at every alpha (k_anchor_col, with llks00), the T best singlets as
// anchors (k_anchor_select), every sample as the partner of every anchor in both orders at n >= 1 (k_anchor_pair), and K3's record over
// what was evaluated (k_anchor_reduce).  The two entry kernels are k_doublet_generic cut down to a wavefront: one wavefront per
// (barcode, slab of 64 NACC entries), tiles of TP = min(32, 64 / A_pad) covered pairs, and per tile
//   phase 1  lane (pair, alpha): pair_values_open / rcp_refined / div_by, the nine finished values to LDS (and, in k_anchor_col's slab 0,
//            the pair's llks00 term);
//   phase 2  lane = entry: the rows of j and k as stored (float32, widened; the products are exact), the nine-term l-major sum from 0.0,
//            dmx_log2, one add — the pairs of a tile in ascending order, so an entry is one serial sum over the barcode's pairs.
// Entries are laid along the lanes with the SAMPLE index fastest (k_anchor_col: (n, j); k_anchor_pair: (t, order, n, k)), so a wavefront
// reads consecutive 12-byte rows and the row of sample 0 / of the anchor is one address.  An entry's operations and operands are those of
// k_doublet_generic's accumulator (j, k, n); nothing in them depends on T, the anchor's rank, the slab or the lane.
// No argument-class test and no fix-up pass: the host refuses a matrix that k_check_geno did not pass.
constexpr int kAncWaves = 4, kAncMaxT = 8, kAncTP = 32;
constexpr uint32_t kAncNone = ~0u;

template <int NACC, bool PAIR>
__device__ __forceinline__ void anchor_body(const PileupView& pv, int nrd_width, const float* __restrict__ g, const double* __restrict__ gp0,
                                            const double* __restrict__ tabs, const double* __restrict__ alpha, int32_t V, int32_t A,
                                            int32_t A_pad, int32_t TP, int32_t T, const int32_t* __restrict__ anchors, int32_t n_slab,
                                            int64_t n_units, double* __restrict__ c0, double* __restrict__ l00, double* __restrict__ pairs) {
  __shared__ double s_tab[kTab2];
  __shared__ double s_pGs[kAncWaves][64 * 9];
  __shared__ double s_t00s[kAncWaves][64];
  __shared__ int32_t s_snps[kAncWaves][kAncTP];
  __shared__ uint32_t s_cnts[kAncWaves][kAncTP];
  __shared__ int64_t s_offs[kAncWaves][kAncTP];
  stage_k2_tables(s_tab, tabs, threadIdx.x, 64 * kAncWaves);
  __syncthreads();
  const double* s_log = s_tab + kLut2;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t unit = (int64_t)blockIdx.x * kAncWaves + wave;
  if (unit >= n_units) return;
  const int32_t cell = (int32_t)(unit / n_slab), slab = (int32_t)(unit % n_slab);
  double* s_pG = s_pGs[wave]; double* s_t00 = s_t00s[wave];
  int32_t* s_snp = s_snps[wave]; uint32_t* s_cnt = s_cnts[wave]; int64_t* s_off = s_offs[wave];

  // this lane's entries: code = (j << 20) | (k << 8) | n, out = where the finished sum goes
  const int64_t n_ent = PAIR ? (int64_t)T * 2 * (A - 1) * V : (int64_t)V * A;
  uint32_t code[NACC];
  int64_t out[NACC];
  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const int64_t en = ((int64_t)slab * NACC + i) * 64 + lane;
    code[i] = kAncNone; out[i] = -1; acc[i] = 0.0;
    if (en >= n_ent) continue;
    const int32_t s = (int32_t)(en % V);
    int32_t r = (int32_t)(en / V);
    if (PAIR) {
      const int32_t n = 1 + r % (A - 1); r /= (A - 1);
      const int32_t o = r & 1, t = r >> 1;
      const int32_t a = anchors[(size_t)cell * T + t];
      out[i] = ((((int64_t)cell * T + t) * V + s) * 2 + o) * (A - 1) + (n - 1);
      if (a >= 0 && a != s) code[i] = ((uint32_t)(o ? s : a) << 20) | ((uint32_t)(o ? a : s) << 8) | (uint32_t)n;
    } else {
      out[i] = ((int64_t)cell * V + s) * A + r;
      code[i] = ((uint32_t)s << 20) | (uint32_t)r;
    }
  }
  const bool do00 = !PAIR && slab == 0;
  double acc00 = 0.0;

  // phase-1 identity and the mixing weights of this lane's alpha (:613)
  const int ti1 = lane / A_pad, n1 = lane % A_pad;
  const bool lane1 = (ti1 < TP) && (n1 < A);
  double wA[9], wR[9];
  {
    const double al = lane1 ? alpha[n1] : 0.0;
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const double p = 0.5 * l + (m - l) * 0.5 * al;
        wA[l * 3 + m] = p;
        wR[l * 3 + m] = 1.0 - p;
      }
  }
  const int64_t p_beg = pv.cell_pair_off[cell];
  const int64_t np = pv.cell_pair_off[cell + 1] - p_beg;
  int64_t rd_base = pv.cell_read_off[cell];
  for (int64_t tbase = 0; tbase < np; tbase += TP) {
    const int tp = (int)min((int64_t)TP, np - tbase);
    load_tile_headers<kAncTP>(pv, nrd_width, p_beg, tbase, tp, lane, rd_base, s_cnt, s_off, s_snp);
    DMX_WAVE_LDS_ORDER();
    rd_base = s_off[tp - 1] + (int64_t)s_cnt[tp - 1];
    // ---- phase 1
    {
      const bool on = lane1 && ti1 < tp;
      const uint32_t cnt = on ? s_cnt[ti1] : 0u;
      const int64_t off = on ? s_off[ti1] : 0;
      const uint32_t rd4 = load_rd4(pv, off, cnt);
      double pG[9];
      const double mx = pair_values_open<9, 0, true>(pv, cnt, off, rd4, s_tab, wA, wR, n1, pG, nullptr, on, A_pad);
      if (on) {
        const double y = rcp_refined(mx);
        double* P = &s_pG[(ti1 * A + n1) * 9];
        if (do00) {
          (void)llks00_term(gp0, s_snp[ti1], [&](int l, int m) { const double v = div_by(pG[l * 3 + m], mx, y); P[l * 3 + m] = v; return v; },
                            s_log, &s_t00[ti1 * A + n1]);
        } else {
#pragma unroll
          for (int i = 0; i < 9; ++i) P[i] = div_by(pG[i], mx, y);                 // :656-663
        }
      }
    }
    DMX_WAVE_LDS_ORDER();
    // ---- phase 2
    for (int ti = 0; ti < tp; ++ti) {
      const int32_t snp = s_snp[ti];
      const float* __restrict__ grow = g + (size_t)snp * V * 3;
#pragma unroll
      for (int i = 0; i < NACC; ++i) {
        const uint32_t cd = code[i];
        if (cd == kAncNone) continue;
        const int32_t j = (cd >> 20) & 0xFFF, k = (cd >> 8) & 0xFFF, n = cd & 0xFF;
        const double a[3] = {(double)grow[j * 3], (double)grow[j * 3 + 1], (double)grow[j * 3 + 2]};
        const double b[3] = {(double)grow[k * 3], (double)grow[k * 3 + 1], (double)grow[k * 3 + 2]};
        const double* P = &s_pG[(ti * A + n) * 9];
        double sum = 0.0;                                                          // :674
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) sum += ((a[l] * b[m]) * P[l * 3 + m]);       // :553 then :677-679, l-major
        acc[i] += dmx_log2_fast(sum, s_log);                                       // :683
      }
      if (do00 && lane < A) acc00 += s_t00[ti * A + lane];                         // :709
    }
    DMX_WAVE_LDS_ORDER();
  }
  double* __restrict__ dst = PAIR ? pairs : c0;
#pragma unroll
  for (int i = 0; i < NACC; ++i)
    if (out[i] >= 0) dst[out[i]] = acc[i];
  if (do00 && lane < A) l00[(size_t)cell * A + lane] = acc00;
}

template <int NACC>
__global__ __launch_bounds__(64 * kAncWaves) void k_anchor_col(PileupView pv, int nrd_width, const float* __restrict__ g, const double* __restrict__ gp0,
                                                             const double* __restrict__ tabs, const double* __restrict__ alpha, int32_t V, int32_t A,
                                                             int32_t A_pad, int32_t TP, int32_t n_slab, int64_t n_units, double* __restrict__ c0,
                                                             double* __restrict__ l00) {
  anchor_body<NACC, false>(pv, nrd_width, g, gp0, tabs, alpha, V, A, A_pad, TP, 0, nullptr, n_slab, n_units, c0, l00, nullptr);
}
template <int NACC>
__global__ __launch_bounds__(64 * kAncWaves) void k_anchor_pair(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                              const double* __restrict__ tabs, const double* __restrict__ alpha, int32_t V, int32_t A,
                                                              int32_t A_pad, int32_t TP, int32_t T, const int32_t* __restrict__ anchors, int32_t n_slab,
                                                              int64_t n_units, double* __restrict__ pairs) {
  anchor_body<NACC, true>(pv, nrd_width, g, nullptr, tabs, alpha, V, A, A_pad, TP, T, anchors, n_slab, n_units, nullptr, nullptr, pairs);
}

__device__ __forceinline__ ArgMax wave_better(ArgMax b) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    ArgMax o;
    o.v = __shfl_xor(b.v, d); o.i = __shfl_xor(b.i, d);
    b = better(b, o);
  }
  return b;
}
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
  return x;
}
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) { const double o = __shfl_xor(x, d); x = (x < o) ? o : x; }
  return x;
}

// The anchors of a barcode: T times the first maximum of sing[j] = c0[j][0] in ascending j among the samples not yet chosen (:746-758,
// repeated).  One wavefront per barcode; a slot stays -1 when no sample is left that compares (NaN likelihoods).
__global__ __launch_bounds__(64 * kAncWaves) void k_anchor_select(const double* __restrict__ c0, int32_t B, int32_t V, int32_t A, int32_t T,
                                                                int32_t* __restrict__ anchors) {
  const int lane = threadIdx.x & 63;
  const int32_t cell = (int32_t)blockIdx.x * kAncWaves + (threadIdx.x >> 6);
  if (cell >= B) return;
  const double* S = c0 + (size_t)cell * V * A;
  int32_t chosen[kAncMaxT];
#pragma unroll
  for (int t = 0; t < kAncMaxT; ++t) chosen[t] = -1;
#pragma unroll
  for (int t = 0; t < kAncMaxT; ++t) {
    if (t >= T) break;
    ArgMax b{-1e300, 0x7FFFFFFF};
    for (int32_t j = lane; j < V; j += 64) {
      bool taken = false;
#pragma unroll
      for (int u = 0; u < kAncMaxT; ++u) taken |= (u < t && chosen[u] == j);
      if (!taken) b = better(b, ArgMax{S[(size_t)j * A], j});
    }
    b = wave_better(b);
    chosen[t] = b.i == 0x7FFFFFFF ? -1 : b.i;
    if (lane == 0) anchors[(size_t)cell * T + t] = chosen[t];
  }
}

// Every evaluated doublet entry (j, k, n) of D_b = {n >= 1, j != k, j an anchor or k an anchor or k = 0} once, strided over the
// wavefront's lanes: column 0 from c0, then the partner rows of every anchor in both orders — skipping (., 0, .) there (it is in c0) and,
// in the order (k, a_t), the rows whose k is itself an anchor (they are that anchor's order (a_u, .)).
template <class F>
__device__ __forceinline__ void anchor_for_each(int lane, int32_t V, int32_t A, int32_t T, const int32_t* s_anc, const double* __restrict__ C0,
                                                const double* __restrict__ PR, F&& f) {
  const int32_t A1 = A - 1;
  for (int32_t e = lane; e < V * A1; e += 64) {
    const int32_t j = e / A1, n = 1 + e % A1;
    if (j != 0) f(j, 0, n, C0[(size_t)j * A + n]);
  }
  const int32_t per_t = V * 2 * A1;
  for (int32_t t = 0; t < T; ++t) {
    const int32_t a = s_anc[t];
    if (a < 0) continue;
    const double* P = PR + (size_t)t * per_t;
    for (int32_t e = lane; e < per_t; e += 64) {
      const int32_t n = 1 + e % A1, r = e / A1, o = r & 1, s = r >> 1;
      if (s == a) continue;
      if (o == 0) {
        if (s != 0) f(a, s, n, P[e]);
      } else {
        bool s_is_anchor = false;
        for (int32_t u = 0; u < T; ++u) s_is_anchor |= (s_anc[u] == s);
        if (a != 0 && !s_is_anchor) f(s, a, n, P[e]);
      }
    }
  }
}

// K3's record (k_reduce) over the evaluated entries.  One wavefront per barcode.  max_llk is the maximum over sing[] and D_b;
// sum_double runs over D_b with the reference's weights; the near-tie flags follow k_reduce's rules over D_b.  A barcode without pairs
// gets the record K3 writes for an all-zero grid.
__global__ __launch_bounds__(64 * kAncWaves) void k_anchor_reduce(const double* __restrict__ c0, const double* __restrict__ pairs,
                                                                const double* __restrict__ l00, const int32_t* __restrict__ anchors,
                                                                const int64_t* __restrict__ cell_pair_off, const double* __restrict__ alpha,
                                                                int32_t B, int32_t V, int32_t A, int32_t T, double prior,
                                                                dmx_cell_summary* __restrict__ out) {
  __shared__ int32_t s_ancs[kAncWaves][kAncMaxT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t cell = (int32_t)blockIdx.x * kAncWaves + wave;
  if (cell >= B) return;
  int32_t* s_anc = s_ancs[wave];
  if (lane < kAncMaxT) s_anc[lane] = lane < T ? anchors[(size_t)cell * T + lane] : -1;
  DMX_WAVE_LDS_ORDER();
  const double* C0 = c0 + (size_t)cell * V * A;
  const double* PR = pairs + (size_t)cell * T * V * 2 * (A - 1);
  const int32_t npairs = (int32_t)(cell_pair_off[cell + 1] - cell_pair_off[cell]);
  dmx_cell_summary r;
  r.n_pairs = npairs; r.reserved = 0; r.llk_ab = 0.0; r.llk_ba = 0.0;
  r.llk_ab_alt = 0.0; r.llk_ba_alt = 0.0; r.ev_x_ab = 0.0; r.ev_t_ab = 0.0; r.ev_x_ba = 0.0; r.ev_t_ba = 0.0;
  if (npairs == 0) {                               // every entry of the grid is 0: k_reduce's scans over it, in closed form
    double ss = 0.0, sd = 0.0;
    for (int32_t j = lane; j < V; j += 64) ss += ((1. - prior) / V);
    for (int32_t n = 1; n < A; ++n) sd += (prior / V / (V - 1) / (A - 1) / (alpha[n] == 0.5 ? 2.0 : 1.0));
    ss = wave_sum(ss);
    sd *= (double)V * (double)(V - 1);
    const int64_t others = (int64_t)V * (V - 1) * (A - 1) - 1 - (alpha[1] == 0.5 ? 1 : 0);
    r.max_llk = 0.0; r.sum_single = ss; r.sum_double = sd;
    r.sing_llk1 = 0.0; r.sing_llk2 = 0.0; r.llk12 = 0.0; r.llk1 = 0.0; r.llk2 = 0.0; r.llk10 = 0.0; r.llk20 = 0.0;
    r.llk00_0 = l00[(size_t)cell * A]; r.llk00_best = l00[(size_t)cell * A + 1];
    r.i_sing1 = 0; r.i_sing2 = 1; r.j_best = 0; r.k_best = 1; r.n_best = 1;
    r.flags = DMX_CELL_NEAR_SINGLET | (others > 0 ? DMX_CELL_NEAR_DOUBLET : 0);
    if (lane == 0) out[cell] = r;
    return;
  }
  // (1) the maximum, the best doublet (first maximum in (j, k, n) scan order, :799-814) and the best singlet (:746-758)
  double mx = -1e300;
  ArgMax bd{-1e300, 0x7FFFFFFF}, b1{-1e300, 0x7FFFFFFF};
  for (int32_t j = lane; j < V; j += 64) {
    const double v = C0[(size_t)j * A];
    mx = fmax(mx, v);
    b1 = better(b1, ArgMax{v, j});
  }
  anchor_for_each(lane, V, A, T, s_anc, C0, PR, [&](int32_t j, int32_t k, int32_t n, double v) {
    mx = fmax(mx, v);
    bd = better(bd, ArgMax{v, (int32_t)(((int64_t)j * V + k) * A + n)});
  });
  const double max_llk = wave_max(mx);
  bd = wave_better(bd); b1 = wave_better(b1);
  const int32_t qbest = bd.i, i1 = b1.i;
  ArgMax b2{-1e300, 0x7FFFFFFF};
  for (int32_t j = lane; j < V; j += 64) if (j != i1) b2 = better(b2, ArgMax{C0[(size_t)j * A], j});
  b2 = wave_better(b2);
  const int32_t i2 = (b2.i == 0x7FFFFFFF) ? -1 : b2.i;
  const bool has1 = i1 != 0x7FFFFFFF, hasb = qbest != 0x7FFFFFFF;
  const int32_t nb = hasb ? qbest % A : 0, jkb = hasb ? qbest / A : 0, jb = jkb / V, kb = jkb % V;
  // (2) posterior sums (:724-734) and the near-tie tests of k_reduce's step (5)
  const double tol = 1e-7;
  const int32_t qmir = (hasb && alpha[nb] == 0.5) ? ((kb * V + jb) * A + nb) : -1;
  const double s2v = (i2 >= 0) ? C0[(size_t)i2 * A] : -1e300, s1v = has1 ? C0[(size_t)i1 * A] : 0.0;
  double ss = 0.0, sd = 0.0;
  int cnt = 0, near_d = 0;
  for (int32_t j = lane; j < V; j += 64) {
    const double v = C0[(size_t)j * A];
    ss += (exp(v - max_llk) * (1. - prior) / V);
    if (v >= s2v - tol) ++cnt;
  }
  anchor_for_each(lane, V, A, T, s_anc, C0, PR, [&](int32_t j, int32_t k, int32_t n, double v) {
    sd += (exp(v - max_llk) * prior / V / (V - 1) / (A - 1) / (alpha[n] == 0.5 ? 2.0 : 1.0));
    const int32_t q = (int32_t)(((int64_t)j * V + k) * A + n);
    if (hasb && q != qbest && q != qmir && v >= bd.v - tol) near_d = 1;
  });
  ss = wave_sum(ss); sd = wave_sum(sd);
  const int n_near_s = (int)wave_sum((double)cnt);
  near_d = __any(near_d) ? 1 : 0;
  int32_t flags = 0;
  if (near_d) flags |= DMX_CELL_NEAR_DOUBLET;
  if (i2 >= 0 && (n_near_s > 2 || s1v - s2v < tol)) flags |= DMX_CELL_NEAR_SINGLET;
  if (lane == 0) {
    const double kNaN = __builtin_nan("");
    r.max_llk = max_llk; r.sum_single = ss; r.sum_double = sd;
    r.i_sing1 = has1 ? i1 : -1; r.i_sing2 = i2;
    r.sing_llk1 = has1 ? s1v : kNaN; r.sing_llk2 = s2v;
    r.j_best = hasb ? jb : -1; r.k_best = hasb ? kb : -1; r.n_best = hasb ? nb : -1;
    r.llk12 = hasb ? bd.v : kNaN;
    r.llk1 = hasb ? C0[(size_t)jb * A] : kNaN; r.llk2 = hasb ? C0[(size_t)kb * A] : kNaN;
    r.llk10 = hasb ? C0[(size_t)jb * A + nb] : kNaN; r.llk20 = hasb ? C0[(size_t)kb * A + nb] : kNaN;     // :824-825
    r.llk00_0 = l00[(size_t)cell * A]; r.llk00_best = l00[(size_t)cell * A + nb];
    if (hasb && has1 && i2 >= 0) {
      const double s1 = r.sing_llk1, s2 = r.sing_llk2;
      if (fabs(r.llk12 - (s1 + 2)) < tol || fabs(s1 - (s2 + 2)) < tol ||
          ((fabs(r.llk12 - r.llk1) < tol || fabs(r.llk12 - r.llk2) < tol) && r.llk12 > s1 + 2 - tol))
        flags |= DMX_CELL_NEAR_RULE;
    }
    r.flags = flags;
    out[cell] = r;
  }
}

// K3b — the tie-order certificate (DESIGN.md "Ties").  At alpha = 0.5 the reference's llksAB[j][k] and llksAB[k][j] are one number
// mathematically and differ by the rounding noise of its own evaluation order; its strict-< scan then names the doublet
// "a-b" or "b-a" by that noise.  To print the same order one has to know BOTH accumulators as the reference computes them, bit for
// bit.  Every operation of the reference except log() is an IEEE operation the device reproduces exactly; for log() the device
// evaluates hi + lo = log(x) in double-double and knows which double(s) a libm with < 0.55 ulp error can return
// (dmx_log_bracket).  One wavefront per barcode re-walks the barcode's pairs for its best alpha = 0.5 pair {a, b} only and
// accumulates, in the reference's order, a LOWER and an UPPER bound of each of the two accumulators (IEEE addition is monotone in
// both operands).  When lower == upper for both, they ARE the reference's values and the order is decided here — for any such
// libm; the host tie arbiter (which calls the host's log()) is left with the barcodes where a bracket stayed open, about one in
// ten.  Requires A = 2 (phase 1 is k_doublet_a2's) and no other doublet entry within 1e-7 of the best (K3's flag).
template <int MINW, bool FIVE, bool DENSE = false>   // FIVE: alpha[0] == 0 (the default grid): five distinct phase-1 values per lane instead of nine;
                                                     // DENSE: gT != NULL (SNP-minor columns) — compile-time strides, so the sparse form's three row entries are one load
__global__ __launch_bounds__(kThreads, MINW) void k_certify(PileupView pv, int nrd_width, const float* __restrict__ g,
                                                      const float* __restrict__ gT,
                                                      const double* __restrict__ tabs, const double* __restrict__ alpha,
                                                      int32_t V, dmx_cell_summary* __restrict__ summ,
                                                      const int64_t* __restrict__ blk, int32_t blk_i, int32_t nblk, double* __restrict__ park,
                                                      const double* __restrict__ cseed, const double* __restrict__ cfin) {
  // blk != nullptr (round 4): this launch covers SNP block blk_i of nblk only — sparse pileups whose genotype matrix does not fit an XCD's L2
  // gather two pieces of a V*12-byte row per pair, and walking the SNP axis block by block (launch_certify; the table is k_snp_blocks',
  // shared with sparse K1) keeps the rows a launch touches L2-resident.  Between launches a barcode's state — the four chains, the open
  // events, the two clean flags, the class-test flag — is parked in park[cell][kPark]; the chains add the same terms in the same order.
  constexpr int TP = 32, T00 = TP + 2, TPC = 64, CPW = kThreads / TPC;
  __shared__ double s_tab[kTab];
  __shared__ double s_lo[128];
  __shared__ __attribute__((aligned(16))) double s_t[CPW][6][T00];   // [ab_lo | ab_hi | ba_lo | ba_hi | ab_x | ba_x][pair]
  __shared__ double s_p[CPW][4][T00];                                // the four chains before each step of the tile (+ after the last)
  __shared__ double s_ev[CPW][4];
  __shared__ int64_t s_offs[CPW][TP];
  __shared__ int32_t s_snps[CPW][TP];
  __shared__ uint32_t s_cnts[CPW][TP];
  const int t = threadIdx.x;
  for (int i = t; i < kTab; i += kThreads) s_tab[i] = tabs[i];
  if (t < 128) s_lo[t] = tabs[kTabLogLo + t];
  __syncthreads();
  const double* s_log = s_tab + kLut;
  const int cw = t / TPC, tid = t % TPC;
  const int32_t cell = blockIdx.x * CPW + cw;
  if (cell >= pv.B) return;
  // only the five words the walk needs stay live (wave-uniform); the record itself is rewritten in place by lane 0
  const int32_t sm_np = summ[cell].n_pairs, sm_j = __builtin_amdgcn_readfirstlane(summ[cell].j_best),
                sm_k = __builtin_amdgcn_readfirstlane(summ[cell].k_best), sm_n = summ[cell].n_best, sm_fl = summ[cell].flags;
  if (sm_np <= 0 || sm_j < 0 || sm_k < 0 || sm_n != 1 || alpha[1] != 0.5 || (sm_fl & DMX_CELL_NEAR_DOUBLET)) return;
  const int32_t ia = min(sm_j, sm_k), ib = max(sm_j, sm_k);
  int64_t* s_off = s_offs[cw]; int32_t* s_snp = s_snps[cw]; uint32_t* s_cnt = s_cnts[cw];
  // (blk_i = first table block of this launch | blocks per launch << 16: a launch may cover several of K1's blocks)
  const int32_t b0 = blk_i & 0xFFFF, bs = max(1, blk_i >> 16), b1 = min(b0 + bs, nblk);
  const int64_t* bt = blk ? blk + ((size_t)cell * (nblk + 1) + b0) * 2 : nullptr;
  const int64_t p_beg = blk ? bt[0] : pv.cell_pair_off[cell];
  const int64_t np = (blk ? bt[2 * (b1 - b0)] : pv.cell_pair_off[cell + 1]) - p_beg;
  int64_t rd_base = blk ? bt[1] : pv.cell_read_off[cell];
  const bool resume = blk && b0 > 0, last_launch = !blk || b1 == nblk;
  double* const pk = park ? park + (size_t)cell * kPark : nullptr;
  const int ti1 = tid >> 1, n1 = tid & 1;
  constexpr bool five = FIVE;
  double wA5[5], wR5[5];
  {
#pragma unroll
    for (int q = 0; q < 5; ++q) {                  // alpha 0.5: p = 0.25 (l + m), slot l + m; alpha 0: p = 0.5 l, slots 0..2 (3, 4 repeat 2)
      const int l = n1 ? (q > 2 ? 2 : q) : min(q, 2), m = n1 ? q - l : 0;
      const double p = 0.5 * l + (m - l) * 0.5 * (n1 ? 0.5 : 0.0);
      wA5[q] = p;
      wR5[q] = 1.0 - p;
    }
  }
  bool ok = resume ? pk[10] != 0.0 : true;
  // Lanes 0..3 own the four chains: (a,b) low, (a,b) high, (b,a) low, (b,a) high = the accumulator had every ambiguous log() come
  // out low / high.  While low == high an accumulator is known.  A step that splits them is an EVENT (its log() argument and
  // lower candidate are kept); from there on each of the two paths has to stay unambiguous by itself (clean): then the
  // reference's value is the low path if its libm returned the lower candidate at the event and the high path otherwise,
  // whatever it returned elsewhere.  The chains are serial (one add per pair); the event / clean tests of a tile's 32 steps
  // run lane-parallel on the chains' prefixes.
  double acc = (resume && tid < 4) ? pk[tid] : 0.0;
  bool clean[2] = {resume ? pk[8] != 0.0 : true, resume ? pk[9] != 0.0 : true};
  if (tid < 4) s_ev[cw][tid] = resume ? pk[4 + tid] : 0.0;   // [ab: log argument, lower candidate | ba: ...] of the open event
  const size_t S = (size_t)pv.S;
  // lane n1 = 0 accumulates llksAB[a][b], lane 1 llksAB[b][a]: the lane's FIRST sample (rows l of :675-681) is a resp. b, its second b resp. a —
  // chosen here, once, by the column pointers instead of per product by selects
  const float* const colA = DENSE ? gT + (size_t)((n1 ? ib : ia) * 3) * S : g + (size_t)(n1 ? ib : ia) * 3;
  const float* const colB = DENSE ? gT + (size_t)((n1 ? ia : ib) * 3) * S : g + (size_t)(n1 ? ia : ib) * 3;
  const size_t estride = DENSE ? S : 1, sstride = DENSE ? 1 : (size_t)V * 3;
  uint32_t hd_n = 0u; int32_t hd_s = 0;          // header (stored reads, SNP id) of this lane's pair in the NEXT tile
  if (tid < TP && tid < np) { hd_n = load_nrd(pv.pair_nrd, p_beg + tid, nrd_width); hd_s = pv.pair_snp ? pv.pair_snp[p_beg + tid] : (int32_t)tid; }
  for (int64_t tbase = 0; tbase < np; tbase += TP) {
    const int tp = (int)min((int64_t)TP, np - tbase);
    if (tid < TP) {
      const uint32_t n = hd_n;                     // this tile's header was requested a tile ago; now request the next one's
      const int32_t sn = hd_s;
      const int64_t nx = tbase + TP + tid;
      hd_n = 0u; hd_s = 0;
      if (nx < np) { hd_n = load_nrd(pv.pair_nrd, p_beg + nx, nrd_width); hd_s = pv.pair_snp ? pv.pair_snp[p_beg + nx] : (int32_t)nx; }
      publish_tile_headers<TP>(n, sn, tid, rd_base, s_cnt, s_off, s_snp);
    }
    DMX_WAVE_LDS_ORDER();
    rd_base = s_off[tp - 1] + (int64_t)s_cnt[tp - 1];
    {
      const bool on = ti1 < tp;
      const uint32_t cnt = on ? s_cnt[ti1] : 0u;
      const int64_t off = on ? s_off[ti1] : 0;
      const uint32_t rd4 = load_rd4(pv, off, cnt);       // the first four read bytes in one load (one dependent latency instead of four)
      // The two samples' probabilities at the pair's SNP.  Dense pileups read them from the SNP-minor copy gT[row element][snp]: the
      // 32 pairs of a tile are 32 consecutive SNPs, i.e. one 128-byte line per element, instead of two lines per PAIR out of
      // V*12-byte rows (165 GB through the L2 per launch at the cfg4 shard, profiles/r02_cfg4_fast_pmc_summary.json).  Sparse
      // pileups read the row of the lane's own SNP.
      const size_t so = (size_t)(on ? s_snp[ti1] : 0) * sstride;
      const float fa0 = colA[so], fa1 = colA[so + estride], fa2 = colA[so + 2 * estride];
      const float fb0 = colB[so], fb1 = colB[so + estride], fb2 = colB[so + 2 * estride];
      double v[9];                                 // pG[1][l][m] of the pair (five: v[l + m])
      if constexpr (five) {
        double v5[5];
        // round 6: pairs of up to three tabled reads take their FINAL values from k_build_certify_finals' table (both lanes of a pair the same entry);
        // the walk below runs only in tiles with a deeper pair (wave-uniform branch)
        const int32_t fi = cfin ? certify_final_index(cnt, rd4) : -1;
        if (!__any(fi < 0)) {
          const double* fp = cfin + (size_t)fi * kCFinStride;
          const double2 a = *reinterpret_cast<const double2*>(fp), b = *reinterpret_cast<const double2*>(fp + 2);
          v5[0] = a.x; v5[1] = a.y; v5[2] = b.x; v5[3] = b.y; v5[4] = fp[4];
        } else {                                   // (a tile with a deeper pair: the walk for ALL its lanes, as before)
          certify_pair_values<5>(pv, cnt, off, rd4, s_tab, wA5, wR5, n1, v5, cseed);
        }
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) v[l * 3 + m] = v5[l + m];
      } else {                                     // other alpha[0]: the nine-value form, weights formed here (:613)
        double wA[9], wR[9];
        const double al = alpha[n1];
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            const double p = 0.5 * l + (m - l) * 0.5 * al;
            wA[l * 3 + m] = p;
            wR[l * 3 + m] = 1.0 - p;
          }
        certify_pair_values<9>(pv, cnt, off, rd4, s_tab, wA, wR, n1, v);
      }
      if (on) {
        const double aj[3] = {(double)fa0, (double)fa1, (double)fa2}, bk[3] = {(double)fb0, (double)fb1, (double)fb2};
        double sx = 0.0;                                                     // :674
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            sx += ((aj[l] * bk[m]) * v[l * 3 + m]);                          // :553, :677-679 (aj = this lane's first sample, see colA)
          }
        ok &= __builtin_amdgcn_class(sx, 0x100);
        double lo1, hi1;
        dmx_log_bracket((uint32_t)__double2hiint(sx), (uint32_t)__double2loint(sx), s_log, s_lo, &lo1, &hi1);
        s_t[cw][2 * n1][ti1] = lo1; s_t[cw][2 * n1 + 1][ti1] = hi1; s_t[cw][4 + n1][ti1] = sx;
      }
    }
    DMX_WAVE_LDS_ORDER();
    if (tid < 4) {
      const double* row = &s_t[cw][tid][0];
      double* pre = &s_p[cw][tid][0];
      double a = acc;
      for (int i = 0; i < tp; ++i) { pre[i] = a; a += row[i]; }              // :683, in pair order
      pre[tp] = a;
      acc = a;
    }
    DMX_WAVE_LDS_ORDER();
    {
      const int i = tid & 31, w = tid >> 5;                                  // step i of accumulator w
      bool ev = false, dirty = false;
      if (i < tp) {
        const double lo = s_p[cw][2 * w][i], hi = s_p[cw][2 * w + 1][i], ll = s_p[cw][2 * w][i + 1], hh = s_p[cw][2 * w + 1][i + 1];
        const double tl = s_t[cw][2 * w][i], th = s_t[cw][2 * w + 1][i];
        const double lh = lo + th, hl = hi + tl;
        const bool closed = lo == hi;
        ev = closed && (ll != lh);
        dirty = !closed && !((ll == lh) && (hl == hh));
      }
      const uint64_t evm = __ballot(ev), dm = __ballot(dirty);
#pragma unroll
      for (int w2 = 0; w2 < 2; ++w2) {
        const uint32_t e32 = (uint32_t)(evm >> (32 * w2)), d32 = (uint32_t)(dm >> (32 * w2));
        if (e32) {
          const int e = 31 - __clz((int)e32);                                // the tile's last event of this accumulator
          if (tid == 0) { s_ev[cw][2 * w2] = s_t[cw][4 + w2][e]; s_ev[cw][2 * w2 + 1] = s_t[cw][2 * w2][e]; }
          clean[w2] = (d32 & ~((2u << e) - 1u)) == 0u;                       // no dirty step after it
        } else {
          clean[w2] = clean[w2] && d32 == 0u;
        }
      }
    }
    DMX_WAVE_LDS_ORDER();
  }
  const bool all_ok = __all(ok ? 1 : 0) != 0;
  if (!last_launch) {                             // park the barcode's state for the next SNP block
    DMX_WAVE_LDS_ORDER();
    if (tid < 4) { pk[tid] = acc; pk[4 + tid] = s_ev[cw][tid]; }
    if (tid == 0) { pk[8] = clean[0] ? 1.0 : 0.0; pk[9] = clean[1] ? 1.0 : 0.0; pk[10] = all_ok ? 1.0 : 0.0; }
    return;
  }
  const double ab_lo = __shfl(acc, 0), ab_hi = __shfl(acc, 1), ba_lo = __shfl(acc, 2), ba_hi = __shfl(acc, 3);
  if (tid == 0 && all_ok && !(ab_lo == ab_hi && ba_lo == ba_hi) && (ab_lo == ab_hi || clean[0]) && (ba_lo == ba_hi || clean[1])) {
    dmx_cell_summary* r = summ + cell;
    r->llk_ab = ab_lo; r->llk_ab_alt = ab_hi; r->llk_ba = ba_lo; r->llk_ba_alt = ba_hi;
    r->ev_x_ab = s_ev[cw][0]; r->ev_t_ab = s_ev[cw][1]; r->ev_x_ba = s_ev[cw][2]; r->ev_t_ba = s_ev[cw][3];
    r->flags = sm_fl | DMX_CELL_ORDER_RESOLVABLE;
  }
  if (tid == 0 && all_ok && ab_lo == ab_hi && ba_lo == ba_hi) {
    // the reference's scan (:799-814, strict <) meets (a,b) before (b,a): it keeps (a,b) unless (b,a) is strictly larger
    const bool ba = ab_lo < ba_lo;
    dmx_cell_summary* r = summ + cell;
    const int32_t nj = ba ? ib : ia, nk = ba ? ia : ib;
    if (nj != sm_j) {
      const double l1 = r->llk1, l2 = r->llk2, l10 = r->llk10, l20 = r->llk20;
      r->llk1 = l2; r->llk2 = l1; r->llk10 = l20; r->llk20 = l10;
    }
    r->j_best = nj; r->k_best = nk;
    r->llk12 = ba ? ba_lo : ab_lo;
    r->llk_ab = ab_lo; r->llk_ba = ba_lo; r->llk_ab_alt = ab_lo; r->llk_ba_alt = ba_lo;
    r->flags = sm_fl | DMX_CELL_ORDER_CERTIFIED;
  }
}

}  // namespace

// =====================================================================================================================
struct dmx_engine {
  int32_t V = 0, A = 0, device = 0, mode = 0;
  bool certify = false;        // run k_certify (the host libm's log() was found inside dmx_log_bracket's brackets)
  double prior = 0.5;
  std::vector<double> alpha;
  Stream own_stream; hipStream_t stream = nullptr;   // stream: own_stream or the caller's (dmx_engine_set_stream); not owned
  Stream k1_stream;                              // dmx_engine_run: K1 beside K2 (lowest priority: it fills what K2's last round leaves free)
  Event ev_fork, ev_k1_done;
  DevBuf<double> d_lut;
  DevBuf<double> d_alpha;
  // genotypes
  const float* d_g = nullptr;                    // not owned: d_g_own, a refinement's or M-step's gp' buffer, or the caller's device matrix
  DevBuf<float> d_g_own; int32_t S = 0; DevBuf<double> d_gp0; DevBuf<float> d_gT; DevBuf<double> d_g0T;
  DevBuf<float> d_rows; DevBuf<uint8_t> d_ids; DevBuf<uint32_t> d_idw, d_idd; int32_t nwd2 = 0; int32_t n_classes = 0;   // genotype classes (0 = not usable)
  // pileup
  PileupView pv{}; int32_t nrd_width = 1; int64_t P = 0, R = 0; bool have_pileup = false;   // pv's pointers are not owned: own[] or the caller's device arrays
  DevBuf<void> own[6];                           // device copies of a host pileup (grow-only: a job's ranges reuse them); [5]: gather sources
  DevBuf<int32_t> d_sched;
  int64_t max_cell_pairs = 0;                                         // covered SNPs of the staged pileup's longest barcode
  DevBuf<int32_t> d_bad;                                             // set by k_check_snp_ids
  bool have_gT = false;                                              // d_gT / d_g0T hold the current genotype matrix
  // canonical GT classes (round 4): every called genotype of a --field GT matrix is one of three SNP-independent rows (hi, lo, lo) permuted
  // (bcf_filtered_reader.cpp:397-400); class ids are then 0 / 1 / 2 = that row with hi in place 0 / 1 / 2 and 3 = the SNP's one other row (a missing
  // genotype's HWE row, :381-388), and K1 takes log(GL . row) of the three canonical rows from a table indexed like the GL tables (d_ltab)
  bool canon = false, ltab_valid = false; float can_hi = 0.f, can_lo = 0.f; DevBuf<double> d_ltab; DevBuf<uint8_t> d_oth;
  DevBuf<uint4> d_snprec; bool snprec_valid = false; DevBuf<double> d_ctab; bool ctab_valid = false;   // k_singlet_can's per-SNP records and merged GL / class-log table
  DevBuf<uint8_t> d_clsb; bool clsb_valid = false; uint32_t clsb_stride = 0;                        // k_singlet_canp's per-sample class byte streams (k_build_clsb)
  bool any_oth = false;                                   // some SNP of the canonical-class matrix has a fourth row (k_canon_apply's oth)
  bool off32 = false;                                     // every absolute pair index and read offset of the staged pileup fits 32 bits
  bool reads_padded = false;                              // four bytes past the staged pileup's last read byte are readable (k_singlet_can's unconditional 4-byte loads)
  DevBuf<double> d_cseed; bool cseed_valid = false;      // certify_pair_values' seeds (k_build_certify_seeds; a function of the phred tables)
  DevBuf<double> d_cfin; bool cfin_valid = false;        // ... and its final values for pairs of up to three tabled reads (k_build_certify_finals, round 6)
  DevBuf<double> d_park;                           // k_certify's per-barcode state between the launches of its SNP-blocked walk
  DevBuf<int64_t> d_blk; int32_t blk_shift = 0, blk_n = 0;   // k_snp_blocks table of the staged (sparse) pileup; blk_n = 0: none
  bool geno_safe = false;                                            // every genotype row finite, non-negative, max >= 2^-400 (k_check_geno)
  bool geno_rows_safe = false;                                       // ... as k_check_geno found it, whatever DMX_FORCE_CHECK says (the anchored pass has no checked form to force)
  // host -> device staging of the big pileup arrays: two pinned chunks filled by host threads while the other one is in flight
  PinnedBuf h_stage[2]; Event ev_stage[2]; bool stage_busy[2] = {false, false}; int stage_cur = 0;
  // results
  DevBuf<double> d_llks, d_llk0s, d_grid, d_l00;
  DevBuf<dmx_cell_summary> d_sum;
  DevBuf<uint8_t> d_flag_base;
  uint8_t* d_flag() const { return d_flag_base ? d_flag_base + kFlagHead : nullptr; }   // the flags proper: a view kFlagHead bytes into the buffer
  DevBuf<double> d_sing;
  int32_t out_cells = 0, grid_cells = 0; bool have_grid = false, have_sing = false;   // cells the result buffers hold
  Event ev[8];
  // the last kRing launches of K1 and of K2 / K3 / K3b, bracketed by events on the engine's stream (dmx_engine_mean_kernel_times)
  static constexpr int kRing = 16;
  Event ring_s[kRing][2], ring_d[kRing][4];
  int64_t n_ring_s = 0, n_ring_d = 0; bool ring_certified[kRing] = {};
  bool timed[4] = {false, false, false, false};
  // Experiment switches.  The DMX_* variables that steer kernel selection — kernel experiments, the tests' forced
  // launch geometries — are copied ONCE, at dmx_engine_create, and only when DMX_EXPERIMENTS=1 is in the environment: a stray DMX_*
  // variable in a user's shell never changes which kernel runs, and no launch reads the environment.
  std::unordered_map<std::string, std::string> knobs;
  const char* knob(const char* name) const { if (knobs.empty()) return nullptr; auto it = knobs.find(name); return it == knobs.end() ? nullptr : it->second.c_str(); }
  // what the last run launched (dmx_engine_kernel_names): host function pointers of the K1 / K2 / K3b kernels, and where K1 ran
  const void *k1_fn = nullptr, *k2_fn = nullptr, *k3b_fn = nullptr; int32_t k1_placement = 0;
  bool k2_sym = false;                                               // launch_doublet picked a k_doublet_sym form (FAST, soft fields, grid {0, 0.5})
  // genotype refinement (dmx_engine_refine_genotypes): its own slab table of the staged pileup (K1's d_blk is not touched), the chunk plan,
  // the partials of one wave, the results; two gp' buffers, so that a refinement never overwrites the matrix the engine was handed by pointer
  DevBuf<int64_t> d_rblk; bool rblk_valid = false; int32_t rblk_S = 0;
  DevBuf<int32_t> d_rplan; std::vector<int32_t> h_rplan;
  DevBuf<RefPartial> d_rpart;
  DevBuf<float> d_rprior;
  DevBuf<double> d_rll;
  DevBuf<int32_t> d_rcnt;
  DevBuf<float> d_rgp[2]; int rgp_cur = -1;
  int32_t ref_S = 0; bool have_refined = false;
  Event rev[4];
  dmx_refine_info ref_info{};
  // genotype-free clustering (dmx_engine_cluster_*): the SNP-major stage cache (a snapshot: staging a pileup again does not touch it),
  // the last E-step's weights and sums, the last M-step's results; two gp' buffers, as for the refinement
  DevBuf<int64_t> d_coff;
  DevBuf<int32_t> d_ccell;
  DevBuf<double> d_clgl;
  DevBuf<uint32_t> d_ccnt;
  int64_t cl_P = 0; int32_t cl_B = 0, cl_S = 0; bool have_cstage = false;
  DevBuf<double> d_cw, d_cwh; bool have_cw = false; int32_t cw_C = 0;
  DevBuf<double> d_clse, d_cpart, d_cpi;         // (an E-step's folded sums are the last row of d_cpart)
  DevBuf<uint8_t> d_cmask;
  DevBuf<double> d_cll, d_cW; DevBuf<float> d_cq;
  DevBuf<float> d_cgp[2]; int cgp_cur = -1; int32_t cm_S = 0, cm_C = 0; bool have_cm = false;
  EventPair cev;
  dmx_cluster_info cl_info{};
  // doublet-aware clustering (dmx_engine_cluster_doublet / _estep_doublet): the pair table, LLD[B][R][P], the per-barcode doublet mass
  // and the host-made log priors; LLD belongs to the staged pileup (staging again drops it)
  DevBuf<uint32_t> d_cpairs;
  DevBuf<double> d_clld;
  DevBuf<double> d_cdm;
  DevBuf<double> d_clp;
  int32_t cd_B = 0, cd_R = 0, cd_K = 0; bool have_cdbl = false;
  EventPair dev_;
  dmx_cluster_doublet_info cd_info{};
  // split-merge moves (dmx_engine_cluster_merge_score / _estep_grouped): the marginals A[S][C] and flags of the last M-step, the
  // prior, the per-chunk partials and the folded scores; the group of each barcode
  DevBuf<double> d_smA;
  DevBuf<uint8_t> d_smF;
  DevBuf<float> d_smq;
  DevBuf<double> d_smpart;
  DevBuf<int32_t> d_smnpart;
  DevBuf<double> d_smout;
  DevBuf<int32_t> d_smnout;
  DevBuf<int32_t> d_cgrp;
  EventPair sev;
  dmx_cluster_sm_info sm_info{};
  // choosing the number of clusters (dmx_engine_cluster_evidence / _hard / _merge_columns): the evidence's partials and folded sums,
  // the hard labels, doublet scores and one-hot matrix [B][C] (a buffer of its own: the E-step's weights are only read), the sums'
  // partials; cdm_*: whether d_cdm holds the doublet mass of the LAST E-step (cluster_estep_run keeps it)
  DevBuf<double> d_kepart; DevBuf<int32_t> d_kenpart;
  DevBuf<int32_t> d_klab; DevBuf<double> d_kdsc, d_khot;
  DevBuf<uint8_t> d_kact, d_kmask;
  DevBuf<int32_t> d_kipart; DevBuf<double> d_kdpart;
  DevBuf<int32_t> d_kfi;
  int32_t khot_B = 0, khot_C = 0, khot_R = 0; bool have_khot = false, khot_dbl = false;
  int32_t cdm_B = 0, cdm_R = 0; bool have_cdm = false;
  EventPair kkev;
  dmx_cluster_k_info k_info{};
  // partly genotyped pools (dmx_engine_cluster_set_known / _estep_known / _mstep_window): the known rows gk[S][Vk][3], every
  // component's weights [B][R][Vk + M] of the last known-column E-step; cgp_C is the column count of the last M-step's gp' buffer
  DevBuf<float> d_ckn; int32_t ckn_S = 0, ckn_Vk = 0; bool have_ckn = false;
  DevBuf<double> d_ckw; int32_t ckw_B = 0, ckw_R = 0, ckw_K = 0; bool have_ckw = false;
  int32_t cgp_C = 0;
  EventPair kev;
  dmx_cluster_known_info kn_info{};
  // ambient contamination profile (dmx_engine_ambient): its own copies of the inputs and the B x Q results
  DevBuf<int32_t> d_aasg;
  DevBuf<double> d_aamb;
  DevBuf<double> d_agrid;
  DevBuf<double> d_all;
  DevBuf<int32_t> d_acnt;
  int32_t amb_B = 0, amb_Q = 0; bool have_amb = false;
  EventPair aev;
  dmx_ambient_info amb_info{};
  // ambient-aware doublet profile (dmx_engine_ambient_doublet): buffers of its own, so that the last singlet profile stays
  DevBuf<int32_t> d_dcand;
  DevBuf<double> d_damb;
  DevBuf<double> d_dgrid;                        // grid[Q], then alpha[A]
  DevBuf<double> d_dll;
  DevBuf<int32_t> d_dcnt;
  int32_t adbl_B = 0, adbl_C = 0, adbl_A = 0, adbl_Q = 0; bool have_adbl = false;
  EventPair dbev;
  dmx_ambient_doublet_info adbl_info{};
  // triplet profile (dmx_engine_triplet): buffers of its own, so that the ambient profiles stay
  DevBuf<int32_t> d_tbase;
  DevBuf<double> d_tshare;                       // shares[T][3]
  DevBuf<double> d_tll;
  DevBuf<int32_t> d_tcnt;                        // n_snp[B][C][V], then n_read[B][C][V]
  int32_t trip_B = 0, trip_C = 0, trip_T = 0, trip_V = 0; bool have_trip = false;
  EventPair tev;
  dmx_triplet_info trip_info{};
  // anchored doublet search (dmx_engine_doublet_anchored): buffers of its own; d_grid is never touched
  DevBuf<int32_t> d_anc;                         // anchors[B][T]
  DevBuf<double> d_ac0, d_apair, d_al00;         // c0[B][V][A], pairs[B][T][V][2][A-1], llks00[B][A]
  DevBuf<dmx_cell_summary> d_asum;
  bool have_anc = false;
  EventPair anc_ev[3];                           // k_anchor_col (+ k_anchor_select), k_anchor_pair, k_anchor_reduce
  dmx_anchored_info anc_info{};
  // pileup composer (dmx_engine_compose): the recipe, the count pass's numbers, and the composed pileup itself (grow-only, like own[])
  DevBuf<int32_t> d_cmparent; DevBuf<uint64_t> d_cmkeep;
  DevBuf<int64_t> d_cmcnt;                       // pairs[n_out] | reads[n_out] | totals[3]
  DevBuf<uint32_t> d_cmmax;
  DevBuf<int64_t> d_cmpoff, d_cmroff;
  DevBuf<int32_t> d_cmsnp; DevBuf<uint8_t> d_cmnrd, d_cmreads;
  bool have_comp = false;
  EventPair cmev[3];
  dmx_compose_info comp_info{};
  // donor shares of a read pool (dmx_engine_census_step / dmx_engine_census): the dosage table d[S][V] and the SNPs' valid flags, the
  // group-sorted cell list and its chunks, the shares and active flags of a pass, the chunk partials and the folded results; the
  // last driver run's results stay on the host
  DevBuf<double> d_cnd; DevBuf<uint8_t> d_cnvalid;
  DevBuf<int32_t> d_cnorder, d_cnoff; DevBuf<CenChunk> d_cnchunk;
  DevBuf<double> d_cnw; DevBuf<uint8_t> d_cnact;
  DevBuf<double> d_cnpart, d_cnout; DevBuf<int64_t> d_cnpcnt, d_cncnt;
  EventPair cnev;
  dmx_census_info cen_info{};
  bool have_cen_info = false, have_census = false;
  int32_t cn_G = 0;
  std::vector<double> cn_w, cn_ll, cn_gap;
  std::vector<int32_t> cn_steps, cn_conv;
  std::vector<int64_t> cn_nread, cn_npair;
  // census uncertainty (dmx_engine_census_fisher): the chunk partials of the information's upper triangle, the folded H[G][V][V], the
  // per-barcode score rows and counted reads
  DevBuf<double> d_fspart, d_fsH, d_fsscore; DevBuf<int64_t> d_fsnb;
  EventPair fsev;
  dmx_census_fisher_info fis_info{};
  bool have_fis_info = false;
  // empirical-Bayes priors (dmx_engine_prior_step / _fit / _call): a caller's host grid copied to the device, the mask, the state
  // pi | d and its log tables, the per-barcode rows, flags and records, the included barcodes' ids and count, the chunk partials and
  // the folded sums; the last step's and fit's results stay on the host
  DevBuf<double> d_prgrid; DevBuf<uint8_t> d_prmask;
  DevBuf<double> d_prst, d_prtab, d_prrows, d_prpart, d_prout;
  DevBuf<uint8_t> d_prflag; DevBuf<dmx_prior_call> d_prcall;
  DevBuf<int32_t> d_pridx, d_prnin;
  EventPair prev[3];                             // k_prior_estep, the fold, k_prior_estep<call>
  dmx_prior_info pr_info{};
  bool have_pr_info = false, have_pr_step = false, have_pr_fit = false, have_pr_call = false;
  int32_t pr_B = 0, pr_V = 0, pr_call_B = 0;
  std::vector<double> pr_step_out;               // N[V] | hom | het | LL | pi'[V] | d' | B_in of the last step
  std::vector<double> pr_fit_out, pr_fit_pi, pr_fit_ll, pr_fit_d;   // ... of the fit's final evaluation; the final pi; the traces
  double pr_fit_dd = 0.0; int32_t pr_fit_iter = 0, pr_fit_conv = 0;
  // goodness of fit (dmx_engine_fit): its own copies of the hypotheses, alpha[B] | rho[B] and a[S], the used barcodes' ids (singlets,
  // then doublets), and the results obs | mean | var [3][B] and n_snp | n_read | n_trunc | n_zero [4][B]
  DevBuf<int32_t> d_fhyp, d_fidx, d_fcnt;
  DevBuf<double> d_fpar, d_famb, d_fout;
  int32_t fit_B = 0; bool have_fit = false;
  EventPair fev;
  dmx_fit_info fit_info{};
  // site audit (dmx_engine_site_fit): its own copies of the hypotheses, alpha[B] | rho[B] and a[S], the plan chunk_beg[n_chunks + 1] |
  // members[n_used], the partials of one wave, and the results obs | mean | var | exc | vexc [5][S] and n_cell | n_read | n_alt |
  // n_trunc | n_zero [5][S]; the slab table is the refinement's d_rblk
  DevBuf<int32_t> d_shyp, d_splan, d_scnt;
  DevBuf<double> d_spar, d_samb, d_sout;
  DevBuf<SitePartial> d_spart;
  int32_t site_S = 0; bool have_site = false;
  EventPair siev;
  dmx_site_fit_info site_info{};
  // model-drawn null pool (dmx_engine_redraw): its own copies of the hypotheses, alpha[B] | rho[B] and a[S], the used barcodes' ids,
  // the per-barcode counts [4][B], and the results: the redrawn read bytes (grow-only, like the composed pileup) and geno[pairs][2]
  DevBuf<int32_t> d_rwhyp, d_rwidx, d_rwcnt;
  DevBuf<double> d_rwpar, d_rwamb;
  DevBuf<uint8_t> d_rwreads; DevBuf<int8_t> d_rwgeno;
  int64_t rw_pairs = 0; bool have_redraw = false;
  EventPair rwev;
  dmx_redraw_info redraw_info{};
  // continuous mixing share (dmx_engine_share_scan / _share_fit): each call's own copies of anchors / cand, rho[B] and a[S], and its
  // results: the scan's (LL, LL', LL'')[B][T][V] and counts [B][T][2]; the fit's 13 doubles and 4 ints per (b, c)
  DevBuf<int32_t> d_ssanc, d_sscnt, d_sfcand, d_sfint;
  DevBuf<double> d_ssrho, d_ssamb, d_ssout, d_sfrho, d_sfamb, d_sfout;
  int32_t ss_B = 0, ss_T = 0, ss_V = 0, sf_B = 0, sf_C = 0; bool have_sscan = false, have_sfit = false;
  EventPair ssev, sfev;
  dmx_share_info share_info{};
  // joint genotype tables (dmx_engine_geno_compare): device copies of host gp matrices and of the weight, the two [S][V][4] images,
  // the invalid rows per column [n_a | n_b], and the table [n_a][n_b][4][4]
  DevBuf<float> d_knga, d_kngb;
  DevBuf<double> d_knw, d_knia, d_knib, d_knt;
  DevBuf<int32_t> d_kncnt;
  std::vector<int32_t> kn_invalid;                 // the host copy of d_kncnt
  bool have_kin = false;
  EventPair knrev, kntev;
  dmx_kin_info kin_info{};
  // block-resolved likelihoods (dmx_engine_block_llk): the call's own copies of block[S] and extra[B][E][3], and its results
  // col[B][G][V], l00[B][G][A], ext[B][G][E] and n_snp[B][G]
  DevBuf<int32_t> d_bkblock, d_bkextra, d_bkn;
  DevBuf<double> d_bkcol, d_bkl00, d_bkext;
  bool have_blk = false;
  EventPair bkev, bkzev;                         // k_block_col; the zeroing before it
  dmx_block_llk_info blk_info{};
};

namespace {

void free_pileup(dmx_engine* e) {
  for (auto& b : e->own) b.reset();
  e->d_sched.reset();
  e->have_pileup = false;
}
void free_results(dmx_engine* e) {
  for (DevBuf<double>* b : {&e->d_llks, &e->d_llk0s, &e->d_grid, &e->d_l00, &e->d_sing}) b->reset();
  e->d_sum.reset(); e->d_flag_base.reset();
  e->out_cells = 0; e->grid_cells = 0; e->have_grid = e->have_sing = false;
}

}  // namespace

namespace { __global__ void k_noop() {} }

extern "C" int dmx_device_warm_up(int32_t device, int32_t n_gpus) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_error(DMX_ERR_NOGPU, "dmx_device_warm_up: no HIP device is visible (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return set_error(DMX_ERR_ARG, "dmx_device_warm_up: device %d of %d", device, ndev);
  for (int i = 0; i < std::max(1, std::min(n_gpus, ndev)); ++i) {
    HIP_TRY(hipSetDevice((device + i) % ndev));
    HIP_TRY(hipFree(nullptr));                   // (creates the primary context)
    hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, nullptr);     // (loads this library's code object onto the device)
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  return DMX_OK;
}

extern "C" int dmx_engine_create(const dmx_engine_config* cfg, dmx_engine** out) {
  if (!cfg || !out) return set_error(DMX_ERR_ARG, "dmx_engine_create: null argument");
  if (cfg->n_samples < 1 || cfg->n_samples > 4094) return set_error(DMX_ERR_ARG, "dmx_engine_create: n_samples %d not in [1,4094]", cfg->n_samples);
  if (cfg->n_alpha < 1 || cfg->n_alpha > 64 || !cfg->alpha) return set_error(DMX_ERR_ARG, "dmx_engine_create: n_alpha %d not in [1,64] or null grid", cfg->n_alpha);
  if (cfg->mode != DMX_MODE_STRICT && cfg->mode != DMX_MODE_FAST) return set_error(DMX_ERR_ARG, "dmx_engine_create: unknown mode %d", cfg->mode);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_error(DMX_ERR_NOGPU, "dmx_engine_create: no HIP device is visible (this library has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return set_error(DMX_ERR_ARG, "dmx_engine_create: device %d of %d", cfg->device, ndev);
  HIP_TRY(hipSetDevice(cfg->device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_error(DMX_ERR_NOGPU, "dmx_engine_create: device %d is %s; this library is built for gfx950 (MI355X) only", cfg->device, prop.gcnArchName);
  std::unique_ptr<dmx_engine> owner(new (std::nothrow) dmx_engine);   // (an early return below frees whatever was created so far)
  dmx_engine* e = owner.get();
  if (!e) return set_error(DMX_ERR_NOMEM, "dmx_engine_create: out of memory");
  e->V = cfg->n_samples; e->A = cfg->n_alpha; e->device = cfg->device; e->mode = cfg->mode; e->prior = cfg->doublet_prior;
  e->alpha.assign(cfg->alpha, cfg->alpha + cfg->n_alpha);
  if (const char* x = getenv("DMX_EXPERIMENTS")) if (x[0] == '1' && !x[1])
    for (char** ev = environ; ev && *ev; ++ev)
      if (!std::strncmp(*ev, "DMX_", 4)) if (const char* eq = std::strchr(*ev, '=')) e->knobs.emplace(std::string((const char*)*ev, (size_t)(eq - *ev)), std::string(eq + 1));
  if (int rc = e->own_stream.create(hipStreamNonBlocking)) return rc;
  e->stream = e->own_stream;
  {
    int least = 0, greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    if (int rc = e->k1_stream.create(hipStreamNonBlocking, least)) return rc;
    if (int rc = e->ev_fork.create(hipEventDisableTiming)) return rc;
    if (int rc = e->ev_k1_done.create(hipEventDisableTiming)) return rc;
  }
  for (Event& ev : e->ev) if (int rc = ev.create()) return rc;
  for (auto& r : e->ring_s) for (Event& ev : r) if (int rc = ev.create()) return rc;
  for (auto& r : e->ring_d) for (Event& ev : r) if (int rc = ev.create()) return rc;
  if (int rc = e->d_lut.alloc(sizeof(double) * kTabTotal)) return rc;
  HIP_TRY(hipMemcpy(e->d_lut + kLut, dmx_log_table_host, sizeof(double) * DMX_LOG_TABLE_DOUBLES, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d_lut + kTabLogLo, dmx_log_table_lo_host, sizeof(double) * 128, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d_lut + kTabLog2, dmx_log2_table_host, sizeof(double) * DMX_LOG2_TABLE_DOUBLES, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d_lut + kTabLog32, dmx_log32_table_host, sizeof(double) * DMX_LOG32_TABLE_DOUBLES, hipMemcpyHostToDevice));
  e->certify = !(cfg->flags & DMX_ENGINE_NO_CERTIFY) && !e->knob("DMX_NO_CERTIFY") && dmx::libm_log_within_brackets();
  if (int rc = e->d_alpha.alloc(sizeof(double) * 64)) return rc;
  HIP_TRY(hipMemcpy(e->d_alpha, e->alpha.data(), sizeof(double) * e->A, hipMemcpyHostToDevice));
  double mat[256], err[256];
  dmx_phred_tables(mat, err);
  if (int rc = dmx_engine_set_phred_tables(e, mat, err)) return rc;
  *out = owner.release();
  return DMX_OK;
}

extern "C" int dmx_engine_destroy(dmx_engine* e) {
  if (!e) return DMX_OK;
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->stream);
  delete e;
  return DMX_OK;
}

extern "C" int dmx_engine_set_stream(dmx_engine* e, void* s) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_set_stream: null engine");
  e->stream = s ? (hipStream_t)s : (hipStream_t)e->own_stream;
  return DMX_OK;
}

extern "C" int dmx_engine_set_phred_tables(dmx_engine* e, const double mat[256], const double err[256]) {
  if (!e || !mat || !err) return set_error(DMX_ERR_ARG, "dmx_engine_set_phred_tables: null argument");
  HIP_TRY(hipSetDevice(e->device));
  dmx::ReadLut lut;
  dmx::build_read_lut(mat, err, &lut);
  HIP_TRY(hipMemcpy(e->d_lut, &lut, sizeof(double) * kLut, hipMemcpyHostToDevice));
  static_assert(sizeof(dmx::SingletTables) == sizeof(double) * (kFirst + kFinal), "table layout");
  dmx::SingletTables st;
  dmx::build_singlet_tables(lut, &st);
  HIP_TRY(hipMemcpy(e->d_lut + kTab, &st, sizeof st, hipMemcpyHostToDevice));
  static_assert(sizeof(dmx::PairTables) == sizeof(double) * 2 * kPair, "table layout");
  std::unique_ptr<dmx::PairTables> pt(new dmx::PairTables);
  dmx::build_pair_tables(lut, st, pt.get());
  HIP_TRY(hipMemcpy(e->d_lut + kTabK1, pt.get(), sizeof(dmx::PairTables), hipMemcpyHostToDevice));
  const dmx::TripleTables& tt = dmx::build_triple_tables(lut, *pt);
  HIP_TRY(hipMemcpy(e->d_lut + kTabK1 + 2 * kPair, tt.third.data(), sizeof(double) * kTriple, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d_lut + kTabK1 + 2 * kPair + kTriple, tt.final3.data(), sizeof(double) * kTriple, hipMemcpyHostToDevice));
  e->ltab_valid = false; e->cseed_valid = false; e->cfin_valid = false; e->ctab_valid = false;   // (the canonical-class log tables and k_certify's seeds are functions of these tables)
  return DMX_OK;
}

extern "C" int dmx_engine_set_genotypes(dmx_engine* e, const float* g, int32_t n_snps, int32_t memory) {
  if (!e || !g || n_snps < 0) return set_error(DMX_ERR_ARG, "dmx_engine_set_genotypes: bad arguments");
  HIP_TRY(hipSetDevice(e->device));
  e->d_g_own.reset(); e->d_gp0.reset();
  e->have_gT = false;
  const size_t n = (size_t)n_snps * e->V * 3;
  if (memory == DMX_MEM_DEVICE) {
    e->d_g = g;
  } else {
    if (int rc = e->d_g_own.alloc(std::max<size_t>(n * sizeof(float), 16))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_g_own, g, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    e->d_g = e->d_g_own;
  }
  e->S = n_snps;
  if (int rc = e->d_gp0.alloc(std::max<size_t>((size_t)n_snps * 3 * sizeof(double), 16))) return rc;
  if (n_snps > 0) {
    const int64_t items = (int64_t)n_snps * 3;
    HIP_TRY(hipEventRecord(e->ev[0], e->stream));
    hipLaunchKernelGGL(k_gp0, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, e->stream, e->d_g, n_snps, e->V, e->d_gp0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e->ev[1], e->stream));
    e->timed[0] = true;
  }

  // genotype classes (<= 4 distinct rows per SNP: --field GT): enables the class kernels
  e->d_rows.reset(); e->d_ids.reset(); e->d_idw.reset(); e->d_idd.reset();
  e->n_classes = 0;
  e->geno_safe = false; e->geno_rows_safe = false;
  if (n_snps > 0) {
    DevBuf<int32_t> d_max, d_unsafe;
    if (int rc = e->d_rows.alloc((size_t)n_snps * kMaxCls * 3 * sizeof(float))) return rc;
    if (int rc = e->d_ids.alloc((size_t)n_snps * e->V + 16)) return rc;
    if (int rc = e->d_idw.alloc((size_t)n_snps * ((e->V + 15) / 16) * sizeof(uint32_t) + 16)) return rc;
    e->nwd2 = ((e->V + e->V / 2 - 1) >> 4) + 5;                     // last window start (V-1 + V/2) >> 4, plus a window of <= 4 words, plus one
    if (int rc = e->d_idd.alloc((size_t)n_snps * e->nwd2 * sizeof(uint32_t) + 16)) return rc;
    if (int rc = d_max.alloc(sizeof(int32_t))) return rc;
    HIP_TRY(hipMemsetAsync(d_max, 0, sizeof(int32_t), e->stream));
    hipLaunchKernelGGL(k_build_classes, dim3((unsigned)((n_snps + 255) / 256)), dim3(256), 0, e->stream, e->d_g, n_snps, e->V,
                       e->d_rows, e->d_ids, e->d_idw, e->d_idd, e->nwd2, d_max);
    HIP_TRY(hipGetLastError());
    if (int rc = d_unsafe.alloc(sizeof(int32_t))) return rc;
    HIP_TRY(hipMemsetAsync(d_unsafe, 0, sizeof(int32_t), e->stream));
    hipLaunchKernelGGL(k_check_geno, dim3(1024), dim3(256), 0, e->stream, e->d_g, (int64_t)n_snps * e->V, d_unsafe);
    HIP_TRY(hipGetLastError());
    int32_t h_max = 0, h_unsafe = 1;
    HIP_TRY(hipMemcpyAsync(&h_max, d_max, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(&h_unsafe, d_unsafe, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    d_max.reset(); d_unsafe.reset();
    e->geno_rows_safe = h_unsafe == 0;
    e->geno_safe = e->geno_rows_safe && !e->knob("DMX_FORCE_CHECK");
    e->n_classes = (h_max >= 1 && h_max <= kMaxCls) ? h_max : 0;
    if (!e->n_classes) { e->d_rows.reset(); e->d_ids.reset(); e->d_idw.reset(); e->d_idd.reset(); }
    // canonical GT classes (see k_canon_apply): relabel when the matrix has that shape
    e->canon = false; e->ltab_valid = false; e->ctab_valid = false; e->snprec_valid = false; e->clsb_valid = false;
    e->d_oth.reset();
    if (e->n_classes && !e->knob("DMX_NO_CANON")) {
      DevBuf<int32_t> d_w;
      if (int rc = d_w.alloc(3 * sizeof(int32_t))) return rc;
      int32_t h_w[3] = {0x7FFFFFFF, 0, 0};
      HIP_TRY(hipMemcpyAsync(d_w, h_w, sizeof h_w, hipMemcpyHostToDevice, e->stream));
      hipLaunchKernelGGL(k_find_canon, dim3((unsigned)((n_snps + 255) / 256)), dim3(256), 0, e->stream, e->d_rows, n_snps, d_w);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(h_w, d_w, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(hipStreamSynchronize(e->stream));
      if (h_w[0] < n_snps) {
        float r[kMaxCls * 3];
        HIP_TRY(hipMemcpy(r, e->d_rows + (size_t)h_w[0] * kMaxCls * 3, sizeof r, hipMemcpyDeviceToHost));
        float hi = 0.f, lo = 0.f; bool found = false;
        for (int d = 0; d < kMaxCls && !found; ++d) {
          const float a = r[d * 3], b = r[d * 3 + 1], c = r[d * 3 + 2];
          uint32_t ua, ub, uc; std::memcpy(&ua, &a, 4); std::memcpy(&ub, &b, 4); std::memcpy(&uc, &c, 4);
          if (!(a >= 0.f && b >= 0.f && c >= 0.f) || !(a < 3e38f && b < 3e38f && c < 3e38f)) continue;
          if (ub == uc && a > b) { hi = a; lo = b; found = true; }
          else if (ua == uc && b > a) { hi = b; lo = a; found = true; }
          else if (ua == ub && c > a) { hi = c; lo = a; found = true; }
        }
        if (found) {
          uint32_t uh, ul; std::memcpy(&uh, &hi, 4); std::memcpy(&ul, &lo, 4);
          hipLaunchKernelGGL(k_canon_check, dim3((unsigned)((n_snps + 255) / 256)), dim3(256), 0, e->stream, e->d_rows, n_snps, uh, ul, d_w + 1);
          HIP_TRY(hipGetLastError());
          HIP_TRY(hipMemcpyAsync(h_w + 1, d_w + 1, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
          HIP_TRY(hipStreamSynchronize(e->stream));
          if (h_w[1] == 0) {
            if (int rc = e->d_oth.alloc((size_t)n_snps + 16)) return rc;
            hipLaunchKernelGGL(k_canon_apply, dim3((unsigned)((n_snps + 255) / 256)), dim3(256), 0, e->stream, e->d_rows, e->d_ids, e->d_idw,
                               e->d_idd, n_snps, e->V, e->nwd2, uh, ul, e->d_oth, d_w + 2);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h_w + 2, d_w + 2, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            e->canon = true; e->can_hi = hi; e->can_lo = lo; e->any_oth = h_w[2] != 0;
          }
        }
      }
    }
  }
  HIP_TRY(hipStreamSynchronize(e->stream));   // the host buffer may go away after return
  return DMX_OK;
}

namespace {

__global__ void k_check_snp_ids(const int32_t* __restrict__ snp, int64_t n, int32_t S, int32_t* __restrict__ bad) {
  bool b = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) b |= (uint32_t)snp[i] >= (uint32_t)S;
  if (b) atomicOr(bad, 1);
}

constexpr size_t kStageBytes = (size_t)16 << 20;

void par_memcpy(uint8_t* dst, const uint8_t* src, size_t n) {
  constexpr size_t kPart = (size_t)2 << 20;
  if (n < 2 * kPart) { std::memcpy(dst, src, n); return; }
  const int T = (int)std::min<size_t>(4, n / kPart);
  std::vector<std::thread> th;
  for (int t = 1; t < T; ++t) th.emplace_back([=] { std::memcpy(dst + n * t / T, src + n * t / T, n * (t + 1) / T - n * t / T); });
  std::memcpy(dst, src, n / T);
  for (std::thread& x : th) x.join();
}

// Streams host bytes into one device array through the engine's two pinned chunks: the host fills one while the copy engine
// drains the other.  (hipMemcpy from pageable memory measured 4 GB/s on this platform; this path is bound by the host memcpy.)
struct StageWriter {
  dmx_engine* e;
  uint8_t* dst;
  size_t fill = 0;
  int slot = 0;
  StageWriter(dmx_engine* e_, void* dst_) : e(e_), dst((uint8_t*)dst_) {}
  int put(const void* src_, size_t n) {
    const uint8_t* src = (const uint8_t*)src_;
    while (n) {
      if (fill == 0) {
        slot = e->stage_cur;
        if (e->stage_busy[slot]) { HIP_TRY(hipEventSynchronize(e->ev_stage[slot])); e->stage_busy[slot] = false; }
      }
      const size_t m = std::min(n, kStageBytes - fill);
      par_memcpy((uint8_t*)e->h_stage[slot].get() + fill, src, m);
      fill += m; src += m; n -= m;
      if (fill == kStageBytes) if (int rc = flush()) return rc;
    }
    return DMX_OK;
  }
  int flush() {
    if (!fill) return DMX_OK;
    HIP_TRY(hipMemcpyAsync(dst, e->h_stage[slot].get(), fill, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipEventRecord(e->ev_stage[slot], e->stream));
    e->stage_busy[slot] = true;
    dst += fill; fill = 0; e->stage_cur ^= 1;
    return DMX_OK;
  }
};

// Cells cells[0..nb) of the host pileup `pl` (NULL = all of them, in order) become cells 0..nb-1 of the engine: the CSR is
// re-based on the fly while it streams to the device, runs of consecutive cells move as one piece.
// A range of a DEVICE-resident pileup whose cells are not consecutive: the cells' pieces of the three big arrays are copied to the
// engine's own buffers on the device (one workgroup per cell; src = the cells' first pair / first read byte in the caller's arrays).
__global__ __launch_bounds__(256) void k_gather_cells(const int64_t* __restrict__ src_pair, const int64_t* __restrict__ src_read,
                                                      const int64_t* __restrict__ dst_pair_off, const int64_t* __restrict__ dst_read_off,
                                                      const int32_t* __restrict__ pair_snp, const uint8_t* __restrict__ pair_nrd, int w,
                                                      const uint8_t* __restrict__ reads, int32_t* __restrict__ o_snp,
                                                      uint8_t* __restrict__ o_nrd, uint8_t* __restrict__ o_reads) {
  const int k = blockIdx.x;
  const int64_t sp = src_pair[k], sr = src_read[k], dp = dst_pair_off[k], dr = dst_read_off[k];
  const int64_t np = dst_pair_off[k + 1] - dp, nr = dst_read_off[k + 1] - dr;
  if (pair_snp) for (int64_t i = threadIdx.x; i < np; i += blockDim.x) o_snp[dp + i] = pair_snp[sp + i];
  for (int64_t i = threadIdx.x; i < np * w; i += blockDim.x) o_nrd[dp * w + i] = pair_nrd[sp * w + i];
  for (int64_t i = threadIdx.x; i < nr; i += blockDim.x) o_reads[dr + i] = reads[sr + i];
}

// dmx_engine_set_pileup for cells cells[0..nb) (NULL: all) of a DEVICE-resident pileup; h_po / h_ro = host copies of its two offset
// arrays.  Consecutive cells are a VIEW of the caller's arrays (nothing is copied: the kernels index the big arrays with the absolute
// offsets they read from cell_pair_off / cell_read_off); anything else is gathered on the device.
int set_pileup_cells_device(dmx_engine* e, const dmx_pileup* pl, const int64_t* h_po, const int64_t* h_ro, const int32_t* cells, int32_t nb,
                            const char* who) {
  const int32_t B = nb;
  const bool dense = !pl->pair_snp && pl->n_pairs > 0;
  bool consecutive = true;
  for (int32_t k = 0; k < B; ++k) {
    const int32_t c = cells ? cells[k] : k;
    if (c < 0 || c >= pl->n_cells) return set_error(DMX_ERR_ARG, "%s: cell %d of %d", who, c, pl->n_cells);
    if (h_po[c + 1] < h_po[c] || h_ro[c + 1] < h_ro[c]) return set_error(DMX_ERR_ARG, "%s: cell_pair_off / cell_read_off not monotone at %d", who, c);
    if (h_po[c] < 0 || h_po[c + 1] > pl->n_pairs || h_ro[c] < 0 || h_ro[c + 1] > pl->n_reads) return set_error(DMX_ERR_ARG, "%s: offsets of cell %d leave the arrays", who, c);
    if (dense && h_po[c + 1] - h_po[c] != pl->n_snps) return set_error(DMX_ERR_ARG, "%s: dense layout needs n_snps pairs per cell (cell %d)", who, c);
    if (cells && k && cells[k] != cells[k - 1] + 1) consecutive = false;
  }
  std::vector<int64_t> h_off((size_t)B + 1, 0), h_roff((size_t)B + 1, 0);
  for (int32_t k = 0; k < B; ++k) {
    const int32_t c = cells ? cells[k] : k;
    h_off[(size_t)k + 1] = h_off[(size_t)k] + (h_po[c + 1] - h_po[c]);
    h_roff[(size_t)k + 1] = h_roff[(size_t)k] + (h_ro[c + 1] - h_ro[c]);
  }
  const int64_t P = h_off[(size_t)B], R = h_roff[(size_t)B];
  if (consecutive) {
    const int32_t c0 = B ? (cells ? cells[0] : 0) : 0;
    e->pv.cell_pair_off = pl->cell_pair_off + c0; e->pv.cell_read_off = pl->cell_read_off + c0;
    e->pv.pair_snp = pl->pair_snp; e->pv.pair_nrd = pl->pair_nrd; e->pv.reads = pl->reads;
    if (!pl->pair_snp && P == 0) {               // no pairs at all: never the dense layout (NULL would select it)
      if (int rc = e->own[2].ensure(16)) return rc;
      e->pv.pair_snp = (const int32_t*)e->own[2].get();
    }
    e->pv.R = pl->n_reads;                       // (the bound of the caller's read array: offsets are absolute in a view)
  } else {
    const size_t w = (size_t)pl->nrd_width;
    if (int rc = e->own[0].ensure(sizeof(int64_t) * ((size_t)B + 1))) return rc;
    if (int rc = e->own[1].ensure(sizeof(int64_t) * ((size_t)B + 1))) return rc;
    if (int rc = e->own[2].ensure(dense ? 16 : sizeof(int32_t) * (size_t)P + 16)) return rc;
    if (int rc = e->own[3].ensure((size_t)P * w + 4)) return rc;
    if (int rc = e->own[4].ensure((size_t)R + 4)) return rc;
    if (int rc = e->own[5].ensure(sizeof(int64_t) * 2 * (size_t)std::max(B, 1))) return rc;
    std::vector<int64_t> src((size_t)2 * std::max(B, 1));
    for (int32_t k = 0; k < B; ++k) { src[(size_t)k] = h_po[cells[k]]; src[(size_t)B + k] = h_ro[cells[k]]; }
    HIP_TRY(hipMemcpyAsync(e->own[0], h_off.data(), sizeof(int64_t) * ((size_t)B + 1), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->own[1], h_roff.data(), sizeof(int64_t) * ((size_t)B + 1), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->own[5], src.data(), sizeof(int64_t) * 2 * (size_t)B, hipMemcpyHostToDevice, e->stream));
    if (B) {
      hipLaunchKernelGGL(k_gather_cells, dim3((unsigned)B), dim3(256), 0, e->stream, (const int64_t*)e->own[5].get(), (const int64_t*)e->own[5].get() + B,
                         (const int64_t*)e->own[0].get(), (const int64_t*)e->own[1].get(), dense ? nullptr : pl->pair_snp, (const uint8_t*)pl->pair_nrd, (int)w,
                         pl->reads, (int32_t*)e->own[2].get(), (uint8_t*)e->own[3].get(), (uint8_t*)e->own[4].get());
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(e->stream));     // (h_off, h_roff, src go away)
    e->pv.cell_pair_off = (const int64_t*)e->own[0].get(); e->pv.cell_read_off = (const int64_t*)e->own[1].get();
    e->pv.pair_snp = (dense && P > 0) ? nullptr : (const int32_t*)e->own[2].get();
    e->pv.pair_nrd = (const uint8_t*)e->own[3].get(); e->pv.reads = (const uint8_t*)e->own[4].get();
    e->pv.R = R;
  }
  if (e->pv.pair_snp && P > 0) {                  // what the kernels will index the genotype matrix with (a view checks its own pairs only)
    if (!e->d_bad) if (int rc = e->d_bad.alloc(sizeof(int32_t))) return rc;
    HIP_TRY(hipMemsetAsync(e->d_bad, 0, sizeof(int32_t), e->stream));
    const int32_t* first = consecutive ? pl->pair_snp + h_po[B ? (cells ? cells[0] : 0) : 0] : e->pv.pair_snp;
    hipLaunchKernelGGL(k_check_snp_ids, dim3(1024), dim3(256), 0, e->stream, first, P, e->S, e->d_bad);
    HIP_TRY(hipGetLastError());
  }
  e->pv.B = B; e->pv.S = e->S; e->nrd_width = pl->nrd_width; e->P = P; e->R = R;
  std::vector<int32_t> sched((size_t)B);
  std::iota(sched.begin(), sched.end(), 0);
  std::stable_sort(sched.begin(), sched.end(), [&](int32_t a, int32_t b) { return (h_off[a + 1] - h_off[a]) > (h_off[b + 1] - h_off[b]); });
  e->max_cell_pairs = B ? h_off[sched[0] + 1] - h_off[sched[0]] : 0;   // (the longest barcode comes first)
  if (int rc = e->d_sched.ensure(sizeof(int32_t) * (size_t)B)) return rc;
  if (B) HIP_TRY(hipMemcpyAsync(e->d_sched, sched.data(), sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, e->stream));
  int32_t bad = 0;
  if (e->pv.pair_snp && P > 0) HIP_TRY(hipMemcpyAsync(&bad, e->d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (bad) return set_error(DMX_ERR_ARG, "%s: a pair_snp entry is outside [0, %d)", who, e->S);
  return DMX_OK;
}

int set_pileup_cells(dmx_engine* e, const dmx_pileup* pl, const int32_t* cells, int32_t nb, const char* who) {
  const int32_t B = nb;
  std::vector<int64_t> h_off((size_t)B + 1, 0), h_roff((size_t)B + 1, 0);
  const bool dense = !pl->pair_snp && pl->n_pairs > 0;
  for (int32_t k = 0; k < B; ++k) {
    const int32_t c = cells ? cells[k] : k;
    if (c < 0 || c >= pl->n_cells) return set_error(DMX_ERR_ARG, "%s: cell %d of %d", who, c, pl->n_cells);
    const int64_t np = pl->cell_pair_off[c + 1] - pl->cell_pair_off[c], nr = pl->cell_read_off[c + 1] - pl->cell_read_off[c];
    if (np < 0 || nr < 0) return set_error(DMX_ERR_ARG, "%s: cell_pair_off / cell_read_off not monotone at %d", who, c);
    if (pl->cell_pair_off[c] < 0 || pl->cell_pair_off[c + 1] > pl->n_pairs || pl->cell_read_off[c] < 0 || pl->cell_read_off[c + 1] > pl->n_reads)
      return set_error(DMX_ERR_ARG, "%s: offsets of cell %d leave the arrays", who, c);
    if (dense && np != pl->n_snps) return set_error(DMX_ERR_ARG, "%s: dense layout needs n_snps pairs per cell (cell %d)", who, c);
    h_off[(size_t)k + 1] = h_off[(size_t)k] + np;
    h_roff[(size_t)k + 1] = h_roff[(size_t)k] + nr;
  }
  const int64_t P = h_off[(size_t)B], R = h_roff[(size_t)B];
  const size_t w = (size_t)pl->nrd_width;
  if (int rc = e->own[0].ensure(sizeof(int64_t) * ((size_t)B + 1))) return rc;
  if (int rc = e->own[1].ensure(sizeof(int64_t) * ((size_t)B + 1))) return rc;
  if (int rc = e->own[2].ensure(dense ? 16 : sizeof(int32_t) * (size_t)P)) return rc;
  if (int rc = e->own[3].ensure((size_t)P * w + 4)) return rc;
  if (int rc = e->own[4].ensure((size_t)R + 4)) return rc;
  for (int i = 0; i < 2; ++i) {
    if (int rc = e->h_stage[i].ensure(kStageBytes)) return rc;
    if (int rc = e->ev_stage[i].create(hipEventDisableTiming)) return rc;
  }
  HIP_TRY(hipMemcpyAsync(e->own[0], h_off.data(), sizeof(int64_t) * ((size_t)B + 1), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->own[1], h_roff.data(), sizeof(int64_t) * ((size_t)B + 1), hipMemcpyHostToDevice, e->stream));
  // the three big arrays, one after the other; a run of consecutive source cells is one contiguous piece of each
  for (int arr = 0; arr < 3; ++arr) {
    if (arr == 0 && dense) continue;
    StageWriter sw(e, e->own[2 + arr]);
    for (int32_t k = 0; k < B;) {
      const int32_t c0 = cells ? cells[k] : k;
      int32_t k1 = k + 1;
      if (!cells) k1 = B; else while (k1 < B && cells[k1] == c0 + (k1 - k)) ++k1;
      const int32_t c1 = c0 + (k1 - k);                                 // source cells [c0, c1)
      const int64_t p0 = pl->cell_pair_off[c0], p1 = pl->cell_pair_off[c1], r0 = pl->cell_read_off[c0], r1 = pl->cell_read_off[c1];
      int rc = DMX_OK;
      if (arr == 0) rc = sw.put(pl->pair_snp + p0, sizeof(int32_t) * (size_t)(p1 - p0));
      else if (arr == 1) rc = sw.put((const uint8_t*)pl->pair_nrd + (size_t)p0 * w, (size_t)(p1 - p0) * w);
      else rc = sw.put(pl->reads + r0, (size_t)(r1 - r0));
      if (rc) return rc;
      k = k1;
    }
    if (int rc = sw.flush()) return rc;
  }
  e->pv.cell_pair_off = (const int64_t*)e->own[0].get(); e->pv.cell_read_off = (const int64_t*)e->own[1].get();
  e->pv.pair_snp = (dense && P > 0) ? nullptr : (const int32_t*)e->own[2].get();   // a range without any pair is sparse with empty cells
  e->pv.pair_nrd = (const uint8_t*)e->own[3].get(); e->pv.reads = (const uint8_t*)e->own[4].get();
  if (!dense && P > 0) {                          // what the kernels will index the genotype matrix with
    if (!e->d_bad) if (int rc = e->d_bad.alloc(sizeof(int32_t))) return rc;
    HIP_TRY(hipMemsetAsync(e->d_bad, 0, sizeof(int32_t), e->stream));
    hipLaunchKernelGGL(k_check_snp_ids, dim3(1024), dim3(256), 0, e->stream, e->pv.pair_snp, P, e->S, e->d_bad);
    HIP_TRY(hipGetLastError());
  }
  e->pv.B = B; e->pv.S = e->S; e->pv.R = R; e->nrd_width = pl->nrd_width; e->P = P; e->R = R;
  // launch order: longest cells first, so the tail of the grid is made of short cells and co-scheduled cells are alike
  std::vector<int32_t> sched((size_t)B);
  std::iota(sched.begin(), sched.end(), 0);
  std::stable_sort(sched.begin(), sched.end(), [&](int32_t a, int32_t b) { return (h_off[a + 1] - h_off[a]) > (h_off[b + 1] - h_off[b]); });
  e->max_cell_pairs = B ? h_off[sched[0] + 1] - h_off[sched[0]] : 0;   // (the longest barcode comes first)
  if (int rc = e->d_sched.ensure(sizeof(int32_t) * (size_t)B)) return rc;
  if (B) HIP_TRY(hipMemcpyAsync(e->d_sched, sched.data(), sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, e->stream));
  int32_t bad = 0;
  if (!dense && P > 0) HIP_TRY(hipMemcpyAsync(&bad, e->d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));       // h_off, h_roff, sched and the caller's arrays may go away after return
  for (int i = 0; i < 2; ++i) e->stage_busy[i] = false;
  if (bad) return set_error(DMX_ERR_ARG, "%s: a pair_snp entry is outside [0, %d)", who, e->S);
  return DMX_OK;
}

}  // namespace

extern "C" int dmx_engine_set_pileup(dmx_engine* e, const dmx_pileup* pl) {
  if (!e || !pl) return set_error(DMX_ERR_ARG, "dmx_engine_set_pileup: null argument");
  return dmx::engine_set_pileup_cells(e, pl, nullptr, pl->n_cells);
}

int dmx::engine_set_pileup_cells(dmx_engine* e, const dmx_pileup* pl, const int32_t* cells, int32_t nb, const int64_t* host_po, const int64_t* host_ro) {
  if (pl->n_cells < 0 || pl->n_pairs < 0 || pl->n_reads < 0 || nb < 0) return set_error(DMX_ERR_ARG, "dmx_engine_set_pileup: negative size");
  if (pl->nrd_width != 1 && pl->nrd_width != 2 && pl->nrd_width != 4) return set_error(DMX_ERR_ARG, "dmx_engine_set_pileup: nrd_width %d", pl->nrd_width);
  if (!pl->cell_pair_off || !pl->cell_read_off || (pl->n_pairs && !pl->pair_nrd) || (pl->n_reads && !pl->reads))
    return set_error(DMX_ERR_ARG, "dmx_engine_set_pileup: missing arrays");
  if (e->S == 0 && pl->n_pairs > 0) return set_error(DMX_ERR_STATE, "dmx_engine_set_pileup: call dmx_engine_set_genotypes first");
  if (pl->n_snps > e->S) return set_error(DMX_ERR_ARG, "dmx_engine_set_pileup: pileup has %d SNPs, genotype matrix %d", pl->n_snps, e->S);
  HIP_TRY(hipSetDevice(e->device));
  e->have_pileup = false;
  const int32_t B = nb;
  if (pl->memory == DMX_MEM_DEVICE) {
    hipPointerAttribute_t at{};                   // the arrays must be visible to this engine's device
    if (hipPointerGetAttributes(&at, pl->cell_pair_off) == hipSuccess && at.type == hipMemoryTypeDevice && at.device != e->device) {
      int can = 0;
      (void)hipDeviceCanAccessPeer(&can, e->device, at.device);
      if (!can) return set_error(DMX_ERR_ARG, "dmx_engine_set_pileup: the pileup lives on device %d, the engine on device %d (no peer access)", at.device, e->device);
    }
    (void)hipGetLastError();
    const int64_t *h_po = host_po, *h_ro = host_ro;
    std::vector<int64_t> po_buf, ro_buf;
    if (!h_po || !h_ro) {
      po_buf.resize((size_t)pl->n_cells + 1); ro_buf.resize((size_t)pl->n_cells + 1);
      HIP_TRY(hipMemcpy(po_buf.data(), pl->cell_pair_off, sizeof(int64_t) * ((size_t)pl->n_cells + 1), hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(ro_buf.data(), pl->cell_read_off, sizeof(int64_t) * ((size_t)pl->n_cells + 1), hipMemcpyDeviceToHost));
      h_po = po_buf.data(); h_ro = ro_buf.data();
    }
    if (!cells && (h_po[0] != 0 || h_po[(size_t)B] != pl->n_pairs)) return set_error(DMX_ERR_ARG, "dmx_engine_set_pileup: cell_pair_off does not span n_pairs");
    if (int rc = set_pileup_cells_device(e, pl, h_po, h_ro, cells, nb, "dmx_engine_set_pileup")) return rc;
  } else {
    if (!cells && (pl->cell_pair_off[0] != 0 || pl->cell_pair_off[(size_t)B] != pl->n_pairs))
      return set_error(DMX_ERR_ARG, "dmx_engine_set_pileup: cell_pair_off does not span n_pairs");
    if (int rc = set_pileup_cells(e, pl, cells, nb, "dmx_engine_set_pileup")) return rc;
  }
  // dense pileups: SNP-minor copies of the genotype probabilities for the singlet kernel (once per genotype matrix)
  if (!e->pv.pair_snp && e->S > 0 && !e->have_gT) {
    e->d_gT.reset(); e->d_g0T.reset();
    if (int rc = e->d_gT.alloc((size_t)e->S * e->V * 3 * sizeof(float))) return rc;
    if (int rc = e->d_g0T.alloc((size_t)e->S * 3 * sizeof(double))) return rc;
    hipLaunchKernelGGL(k_transpose_geno, dim3(2048), dim3(256), 0, e->stream, e->d_g, e->d_gp0, e->S, e->V, e->d_gT, e->d_g0T);
    HIP_TRY(hipGetLastError());
    e->have_gT = true;
  }
  // sparse pileups over a genotype matrix that does not fit the L2: the SNP-block table of the blocked K1 walk (launch_singlet)
  e->blk_n = 0;
  if (e->pv.pair_snp && e->P > 0 && e->S > 0 && !e->knob("DMX_K1_NO_BLOCKS")) {
    const double row_bytes = (double)e->V * 12.0 + 24.0;
    double target = 2.0 * 1024 * 1024;                                  // bytes of genotype rows per block
    const char* env = e->knob("DMX_K1_BLOCK_BYTES");                     // tests / kernel experiments: any block size, no size heuristics
    if (env) target = atof(env);
    int shift = 0;
    while (shift < 30 && (double)(2ll << shift) * row_bytes <= target) ++shift;
    const int32_t nblk = (int32_t)(((int64_t)e->S + (1ll << shift) - 1) >> shift);
    // worth it only when the matrix is well beyond one L2 and a barcode still has a few tiles of pairs per block
    if (nblk > 1 && (env || ((double)e->S * row_bytes > 3.0 * 1024 * 1024 && (double)e->P / std::max(B, 1) / nblk >= 96.0))) {
      if (int rc = e->d_blk.ensure(sizeof(int64_t) * 2 * (size_t)B * (nblk + 1))) return rc;
      hipLaunchKernelGGL(k_snp_blocks, dim3((unsigned)((B + 3) / 4)), dim3(kThreads), 0, e->stream, e->pv, e->nrd_width, shift, nblk, e->d_blk);
      HIP_TRY(hipGetLastError());
      e->blk_shift = shift; e->blk_n = nblk;
    }
  }
  if (e->out_cells < B || !e->d_llks) {
    free_results(e);
    const int32_t cap = B + B / 16 + 16;
    if (int rc = e->d_llks.alloc(sizeof(double) * (size_t)cap * e->V)) return rc;
    if (int rc = e->d_llk0s.alloc(sizeof(double) * (size_t)cap)) return rc;
    e->out_cells = cap;
  }
  // k_singlet_can's preconditions: every ABSOLUTE pair index / read offset the kernels form fits 32 bits (a view of a caller's device arrays
  // indexes the caller's whole arrays), and the four bytes behind the last read byte are readable (the engine's own copies are allocated
  // with slack; a caller's device array is, when its allocation extends that far)
  {
    const bool own_reads = e->pv.reads == (const uint8_t*)e->own[4].get();
    const uint64_t maxP = own_reads ? (uint64_t)e->P : (uint64_t)std::max<int64_t>(pl->n_pairs, e->P);
    const uint64_t maxR = (uint64_t)std::max<int64_t>(e->pv.R, e->R);
    e->off32 = maxP + 4 * 64 < (1ull << 32) && maxR + 64 < (1ull << 32);
    e->reads_padded = own_reads;
    if (!own_reads && e->pv.reads) {
      hipDeviceptr_t base = nullptr; size_t size = 0;
      if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)e->pv.reads) == hipSuccess)
        e->reads_padded = (const uint8_t*)base + size >= e->pv.reads + maxR + 4;
      (void)hipGetLastError();
    }
  }
  e->have_sing = e->have_grid = false;
  e->rblk_valid = false; e->have_refined = false; e->have_amb = false; e->have_adbl = false; e->have_cdbl = false;
  e->have_trip = false;
  e->have_fit = false;
  e->have_site = false;
  e->have_redraw = false;
  e->have_sscan = false; e->have_sfit = false;
  e->have_blk = false;
  e->have_comp = false;
  e->have_census = false; e->have_cen_info = false; e->have_fis_info = false;
  e->have_pileup = true;
  e->k1_fn = e->k2_fn = e->k3b_fn = nullptr; e->k1_placement = 0;      // nothing has run on this pileup yet
  return DMX_OK;
}

namespace {

// Every K1 / K2 / K3b launch goes through these: the engine remembers WHICH kernel it launched (dmx_engine_kernel_names), so that nothing
// outside launch_singlet / launch_doublet / launch_certify re-derives their selection (bench.py pairs its counter files with it).
#define DMX_LAUNCH(SLOT, K, ...) do { e->SLOT = reinterpret_cast<const void*>(&K); hipLaunchKernelGGL(K, __VA_ARGS__); } while (0)
#define DMX_LAUNCH_IF(COND, SLOT, K, ...) do { if (COND) e->SLOT = reinterpret_cast<const void*>(&K); hipLaunchKernelGGL(K, __VA_ARGS__); } while (0)

// k_build_certify_finals' table (round 6), for the kernels that run phase 1 of the default grid {0, 0.5}: k_doublet_sym and k_certify<FIVE>.  Only shallow
// pileups take it — at most 1.6 stored reads per covered pair on average: a tile skips its read loop only when NONE of its 16 / 32 pairs is deeper than
// three reads (1.25 reads per pair: 93 % of the tiles; 2 reads per pair, cfg5: 7 %, and there the look-ups into a table beyond the L2 cost more than
// they save — measured, k_certify 7.57 -> 8.23 ms).  *out stays NULL when the pileup is deeper, or too small to pay for the table.
int ensure_seeds(dmx_engine* e, const double** out) {      // k_build_certify_seeds' table (default grid {0, 0.5}: k_certify<FIVE>, k_doublet_sym)
  if (!e->cseed_valid) {
    if (!e->d_cseed) if (int rc = e->d_cseed.alloc(sizeof(double) * 2 * kCSeedStride * (size_t)kCSeedN)) return rc;
    hipLaunchKernelGGL(k_build_certify_seeds, dim3((unsigned)((kCSeedN + 255) / 256)), dim3(256), 0, e->stream, e->d_lut, e->d_cseed);
    HIP_TRY(hipGetLastError());
    e->cseed_valid = true;
  }
  *out = e->d_cseed;
  return DMX_OK;
}
int ensure_finals(dmx_engine* e, const double** out) {
  *out = nullptr;
  if ((double)e->R > 1.6 * (double)std::max<int64_t>(e->P, 1) && !e->knob("DMX_FINALS_ANY_DEPTH")) return DMX_OK;
  // ... and only jobs big enough to pay for it: allocating and filling the 58 MB table costs an engine ~1.5 ms (cfg6's 0.035 s job: +4 %, measured),
  // what it saves is ~2 ms per 1e8 covered pairs (cfg3, 5e8 pairs: 13 ms STRICT, 7 ms FAST)
  if (e->P < 100000000 && !e->cfin_valid && !e->knob("DMX_FINALS_ANY_DEPTH")) return DMX_OK;
  if (!e->cfin_valid) {
    if (!e->d_cfin) if (int rc = e->d_cfin.alloc(sizeof(double) * kCFinStride * (size_t)kCFinN)) return rc;
    hipLaunchKernelGGL(k_build_certify_finals, dim3((unsigned)((kCFinN + 255) / 256)), dim3(256), 0, e->stream, e->d_lut, e->d_cfin);
    HIP_TRY(hipGetLastError());
    e->cfin_valid = true;
  }
  *out = e->d_cfin;
  return DMX_OK;
}

int launch_singlet(dmx_engine* e) {
  const int32_t B = e->pv.B, V = e->V;
  // cells per wavefront: more cells amortise the ordered sums, fewer keep >= ~4 wavefronts per SIMD in flight (1024 SIMDs)
  int CW = (B >= 64 * 1024) ? 4 : (B >= 24 * 1024 ? 2 : 1);
  const int KC = (V <= 4) ? 4 : 8;
  if (const char* cenv = e->knob("DMX_K1_CW")) CW = atoi(cenv);     // kernel experiments only
  if (e->n_classes > 0 && !e->knob("DMX_NO_CLASSES") && !e->knob("DMX_NO_K1_CLASSES")) {
    // --field GT inputs: log() once per genotype class instead of once per sample (bit-identical, see k_singlet_cls)
    const int wide_v = e->knob("DMX_K1_WIDE_V") ? atoi(e->knob("DMX_K1_WIDE_V")) : 20;      // kernel experiments only
    if (V >= wide_v && V <= 1024) {              // wide panels: chains look the class terms up themselves, one pass per tile
      const size_t dynw = (size_t)(kThreads / 64) * 64 * ((V + 15) / 16) * sizeof(uint32_t);
      const bool l0m = V % 64 == 0 && !e->knob("DMX_K1W_NO_L0M");     // llk0 merged into the first pass instead of a pass of its own (k_singlet_clsw)
      const dim3 blkw(kThreads), grdw((unsigned)((B + (kThreads / 64) - 1) / (kThreads / 64)), (unsigned)((V + (l0m ? 0 : 1) + 255) / 256));
#define DMX_K1W(...) do {                                                                                                          \
      if (dynw > 30 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_singlet_clsw<__VA_ARGS__>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dynw)); \
      DMX_LAUNCH(k1_fn, (k_singlet_clsw<__VA_ARGS__>), grdw, blkw, dynw, e->stream, e->pv, e->nrd_width, e->d_rows, e->d_idw, e->d_gp0,    \
                         e->d_lut, e->d_sched, V, e->d_llks, e->d_llk0s); } while (0)
      if (e->knob("DMX_K1W_MINW3")) { if (l0m) DMX_K1W(1, 3, true); else DMX_K1W(1, 3, false); }              // kernel experiments only
      else if (l0m) DMX_K1W(1, 4, true);
      else DMX_K1W(1, 4, false);
#undef DMX_K1W
      return DMX_OK;
    }
    // measured on cfg2-shaped inputs (profiles/): CW 2 wins from 10 k barcodes (6.90 vs 7.14 ms; 5 k: 5.07 vs 3.94).  Four barcodes per wavefront
    // (round 6, profiles/r06_k1_cw4.txt): k_singlet_cls LOSES with them at every size tried — 131 072 barcodes x 50 k SNPs 64.4 against
    // 50.7 ms, 262 144: 127.2 / 100.7 (round 3: 40 k 27.7 / 24.6) — so it never takes them; the lean kernel k_singlet_can gains 2.6 % at 65 536
    // (17.15 / 17.60 ms) and takes them from there (beyond 2^32 covered pairs per engine — 131 072 x 50 k — the lean kernel's 32-bit offsets do not
    // reach and k_singlet_cls runs: DESIGN 10).
    const bool lean_ok = e->canon && e->geno_safe && !e->knob("DMX_NO_CANON_K1") && V <= 16 && e->nrd_width == 1 && e->reads_padded && e->off32 &&
                         (uint64_t)e->S * 64 < (1ull << 32) && !e->knob("DMX_K1_NO_LEAN");       // (the conditions of `lean` below)
    if (!e->knob("DMX_K1_CW")) CW = (lean_ok && B >= 64 * 1024) ? 4 : (B >= 10000 ? 2 : 1);
    const int nchc = (V + KC - 1) / KC;
    const size_t dynb = sizeof(double) * (size_t)(kThreads / 64) * nchc * CW * (KC + 1);
    if (dynb <= 16 * 1024) {
      const dim3 blk(kThreads), grd((unsigned)((B + (kThreads / 64) * CW - 1) / ((kThreads / 64) * CW)));
      const int chk = e->geno_safe ? 0 : 1;       // (DMX_FORCE_CHECK=1 keeps the test: bit-identical, tests/test_gpu_parity.py)
      // canonical GT classes: three of a pair's five log terms from the table (k_singlet_cls<.., CAN>; DMX_NO_CANON_K1=1: the plain class form)
      const bool can = e->canon && chk == 0 && !e->knob("DMX_NO_CANON_K1");
      // the lean canonical-class kernel (round 5): one id word per SNP, one-byte read counts, every offset in 32 bits, padded read bytes
      const bool lean = can && V <= 16 && e->nrd_width == 1 && e->reads_padded && e->off32 && (uint64_t)e->S * 64 < (1ull << 32) && !e->knob("DMX_K1_NO_LEAN");
      if (lean) {
        if (!e->snprec_valid) {
          if (int rc = e->d_snprec.alloc(kSnpRecBytes * (size_t)std::max(e->S, 1))) return rc;
          hipLaunchKernelGGL(k_build_snprec, dim3((unsigned)((e->S + 255) / 256)), dim3(256), 0, e->stream, e->d_gp0, e->d_ids, e->d_oth, e->S, V, e->d_snprec);
          HIP_TRY(hipGetLastError());
          e->snprec_valid = true;
        }
        if (!e->ctab_valid) {
          if (!e->d_ctab) if (int rc = e->d_ctab.alloc(sizeof(double) * 8 * (size_t)kCtN)) return rc;
          hipLaunchKernelGGL(k_build_ctab, dim3((unsigned)((kCtN + 255) / 256)), dim3(256), 0, e->stream, e->d_lut, (double)e->can_hi, (double)e->can_lo, e->d_ctab);
          HIP_TRY(hipGetLastError());
          e->ctab_valid = true;
        }
        // (a matrix with a fourth genotype row somewhere — missing genotypes — keeps four class planes of scratch and gathers every entry from the
        //  global table; without one the commonest entries come from an LDS copy: see the kernel)
        const bool oth = e->any_oth;
        // dense pileups of up to 8 samples without a fourth genotype row (cfg2): producers / consumer (k_singlet_canp) — an EXPERIMENT (DMX_K1_CANP=1), bit-identical
        // and not faster: cfg2 3.34 ms at three workgroups per CU against k_singlet_can's 3.15 (4.11 at two, 7.8 at four with spills).  Its consumer does what
        // it was built for (64 ordered steps of sdwa-add / ds_read / add for 448 pairs), but a producer's own per-tile work — scan, table index, look-up, llk0 log:
        // ~120 VALU instructions — is what both kernels are made of, and both wait for the same two HBM streams (timing builds without the read-count and
        // read-byte loads: 2.31 and 2.71 ms; touching those lines 4 / 8 / 16 tiles ahead from the consumer's spare lanes: 3.44-3.50 ms, no help) — DESIGN 11.
        if (!oth && V <= 8 && e->pv.pair_snp == nullptr && e->knob("DMX_K1_CANP") && !e->knob("DMX_K1_NO_CANP") && !e->knob("DMX_K1_CW")) {
          if (!e->clsb_valid) {
            e->clsb_stride = (uint32_t)(((int64_t)e->S + 63) / 64 * 64 + 64);
            if (int rc = e->d_clsb.alloc((size_t)9 * e->clsb_stride)) return rc;
            hipLaunchKernelGGL(k_build_clsb, dim3((unsigned)(((size_t)9 * e->clsb_stride + 255) / 256)), dim3(256), 0, e->stream, e->d_ids, e->S, V, e->clsb_stride, e->d_clsb);
            HIP_TRY(hipGetLastError());
            e->clsb_valid = true;
          }
          const dim3 grdp((unsigned)((B + kCpB - 1) / kCpB));
          if (e->knob("DMX_K1_CANP_MINW4"))        // kernel experiments only (two workgroups per CU)
            DMX_LAUNCH(k1_fn, (k_singlet_canp<4>), grdp, dim3(kCpThreads), 0, e->stream, e->pv, e->d_snprec, e->d_clsb, e->clsb_stride, e->d_ctab, e->d_lut, e->d_sched, V,
                               e->d_llks, e->d_llk0s, (double)e->can_hi, (double)e->can_lo);
          else
            DMX_LAUNCH(k1_fn, (k_singlet_canp<6>), grdp, dim3(kCpThreads), 0, e->stream, e->pv, e->d_snprec, e->d_clsb, e->clsb_stride, e->d_ctab, e->d_lut, e->d_sched, V,
                               e->d_llks, e->d_llk0s, (double)e->can_hi, (double)e->can_lo);
          return DMX_OK;
        }
#define DMX_K1L_(CC, KK, OO, NN) DMX_LAUNCH(k1_fn, (k_singlet_can<CC, KK, OO, NN>), grd, blk, 0, e->stream, e->pv, e->d_snprec, e->d_rows, e->d_ctab, e->d_lut, e->d_sched, V, \
                                            e->d_llks, e->d_llk0s, (double)e->can_hi, (double)e->can_lo)
#define DMX_K1L(CC, KK, NN) do { if (oth) DMX_K1L_(CC, KK, true, NN); else DMX_K1L_(CC, KK, false, NN); } while (0)
        if (KC == 4) { if (CW == 4) DMX_K1L(4, 4, 1); else if (CW == 2) DMX_K1L(2, 4, 1); else DMX_K1L(1, 4, 1); }
        else if (nchc == 1) { if (CW == 4) DMX_K1L(4, 8, 1); else if (CW == 2) DMX_K1L(2, 8, 1); else DMX_K1L(1, 8, 1); }
        else                { if (CW == 4) DMX_K1L(4, 8, 2); else if (CW == 2) DMX_K1L(2, 8, 2); else DMX_K1L(1, 8, 2); }
#undef DMX_K1L
#undef DMX_K1L_
        return DMX_OK;
      }
      if (can && !e->ltab_valid) {
        if (!e->d_ltab) if (int rc = e->d_ltab.alloc(sizeof(double) * 4 * (size_t)kCanN)) return rc;
        hipLaunchKernelGGL(k_build_canon_logs, dim3((unsigned)((kCanN + 255) / 256)), dim3(256), 0, e->stream, e->d_lut, (double)e->can_hi,
                           (double)e->can_lo, e->d_ltab);
        HIP_TRY(hipGetLastError());
        e->ltab_valid = true;
      }
#define DMX_K1C_(CC, KK, CAN_) DMX_LAUNCH(k1_fn, (k_singlet_cls<CC, KK, CAN_>), grd, blk, dynb, e->stream, e->pv, e->nrd_width, e->d_rows, chk, \
                                           e->d_idw, e->d_gp0, e->d_lut, e->d_sched, V, e->d_llks, e->d_llk0s, e->d_ltab, e->d_oth,           \
                                           (double)e->can_hi, (double)e->can_lo)
#define DMX_K1C(CC, KK) do { if (can) DMX_K1C_(CC, KK, true); else DMX_K1C_(CC, KK, false); } while (0)
      if (KC == 4) { if (CW == 4) DMX_K1C(4, 4); else if (CW == 2) DMX_K1C(2, 4); else DMX_K1C(1, 4); }
      else         { if (CW == 4) DMX_K1C(4, 8); else if (CW == 2) DMX_K1C(2, 8); else DMX_K1C(1, 8); }
#undef DMX_K1C
#undef DMX_K1C_
      return DMX_OK;
    }
  }
  const int nch = (V + KC - 1) / KC;
  const int NW = kThreads / 64;
  const int QS = std::min(nch, (int)(16 * 1024 / (sizeof(double) * (size_t)NW * CW * (KC + 1))));   // chunks per workgroup: 16 KB of sums
  const unsigned q_slabs = (unsigned)((nch + QS - 1) / QS);
  const size_t dyn = sizeof(double) * (size_t)NW * QS * CW * (KC + 1);
  const bool dense = e->pv.pair_snp == nullptr;
  if (dense && (size_t)e->S * V * 12 > 0x7FFFFFFFull) return set_error(DMX_ERR_ARG, "run_singlet: dense genotype matrix over 2 GiB is not supported by this build");
  const float* gq = dense ? e->d_gT : e->d_g;
  const double* g0q = dense ? e->d_g0T : e->d_gp0;
  const dim3 block(kThreads), grid((unsigned)((B + NW * CW - 1) / (NW * CW)), q_slabs);
  // Sparse pileups gather one genotype row per covered pair; when the matrix is larger than an XCD's L2 (4 MB) nearly every row
  // comes out of the Infinity Cache (cfg5: 56 GB per launch for 1.5 GB of algorithmic bytes, profiles/r02_cfg5_pmc_summary.json).
  // The SNP axis is then walked in blocks of 2^blk_shift SNPs (about 2 MB of rows), one launch per block over all barcodes: the
  // rows of a launch stay L2-resident; the sums are parked in llks / llk0s between launches (see the kernel).
  const int64_t* blk = (!dense && e->blk_n > 1) ? e->d_blk : nullptr;
  const int n_launch = blk ? e->blk_n : 1;
  // soft fields, 9..64 samples: the kernel whose lanes own their samples' sums (k_singlet_own; DMX_K1_NO_OWN=1: k_singlet, bit-identical)
  if (V >= 9 && V <= 64 && (size_t)e->S * V * 12 <= 0x7FFFFFFFull && !e->knob("DMX_K1_NO_OWN")) {
    const int tpc = V <= 16 ? 16 : (V <= 32 ? 32 : 64);
    const int cwo = 64 / tpc;
    const dim3 grd((unsigned)((B + NW * cwo - 1) / (NW * cwo)));
    const bool chk = !e->geno_safe || e->knob("DMX_FORCE_CHECK");
#define DMX_K1O_(TT, DD, CC)                                                                                           \
    for (int bi_ = 0; bi_ < n_launch; ++bi_)                                                                           \
      DMX_LAUNCH(k1_fn, (k_singlet_own<TT, DD, CC>), grd, block, 0, e->stream, e->pv, e->nrd_width, e->d_g, e->d_gp0, e->d_lut, \
                         e->d_sched, V, e->d_llks, e->d_llk0s, blk, bi_, e->blk_n)
#define DMX_K1O(TT) do { if (dense) { if (chk) DMX_K1O_(TT, true, true); else DMX_K1O_(TT, true, false); }            \
                         else { if (chk) DMX_K1O_(TT, false, true); else DMX_K1O_(TT, false, false); } } while (0)
    if (tpc == 16) DMX_K1O(16); else if (tpc == 32) DMX_K1O(32); else DMX_K1O(64);
#undef DMX_K1O
#undef DMX_K1O_
    return DMX_OK;
  }
#define DMX_K1(CC, KK, DD)                                                                                            \
  for (int bi_ = 0; bi_ < n_launch; ++bi_)                                                                             \
    DMX_LAUNCH(k1_fn, (k_singlet<CC, KK, DD>), grid, block, dyn, e->stream, e->pv, e->nrd_width, gq, g0q, e->d_lut,   \
                       e->d_sched, V, QS, e->d_llks, e->d_llk0s, blk, bi_, e->blk_n)
#define DMX_K1_D(CC, KK) do { if (dense) DMX_K1(CC, KK, true); else DMX_K1(CC, KK, false); } while (0)
  if (KC == 4) { if (CW == 4) DMX_K1_D(4, 4); else if (CW == 2) DMX_K1_D(2, 4); else DMX_K1_D(1, 4); }
  else         { if (CW == 4) DMX_K1_D(4, 8); else if (CW == 2) DMX_K1_D(2, 8); else DMX_K1_D(1, 8); }
#undef DMX_K1_D
#undef DMX_K1
  return DMX_OK;
}

template <typename NRD, bool FIXUP>
int launch_doublet_generic(dmx_engine* e) {
  const int32_t B = e->pv.B, V = e->V, A = e->A;
  int A_pad = 1;
  while (A_pad < A) A_pad <<= 1;
  const int TP = std::min(32, kThreads / A_pad);
  const int64_t nacc = (int64_t)V * V * A + A;
  const int per = (int)((nacc + kThreads - 1) / kThreads);
  if (nacc > 0x7FFFFFFFll || V > 0xFFE) return set_error(DMX_ERR_ARG, "run_doublet: V*V*A = %lld accumulators per cell exceed this build's limit", (long long)nacc);
  const int slab_acc = 33;                        // accumulators per thread when the grid is cut into slabs
  const unsigned slabs = per <= 65 ? 1u : (unsigned)((nacc + (int64_t)slab_acc * kThreads - 1) / ((int64_t)slab_acc * kThreads));
  if (slabs > 65535u) return set_error(DMX_ERR_ARG, "run_doublet: V*V*A = %lld accumulators per cell exceed this build's limit (5.5e8)", (long long)nacc);
  // the fix-up pass strides a fixed grid over the cells (see the kernel); the first pass has one workgroup per cell
  const dim3 grid(FIXUP ? (unsigned)std::min(B, 256) : (unsigned)B, slabs), block(kThreads);
#define DMX_K2(NN)                                                                                                   \
  DMX_LAUNCH_IF(!FIXUP, k2_fn, (k_doublet_generic<NRD, NN, FIXUP>), grid, block, 0, e->stream, e->pv, e->d_g, e->d_gp0, e->d_lut, \
                     e->d_alpha, e->d_sched, V, A, A_pad, TP, e->d_grid, e->d_l00, e->d_flag())
  if (per <= 1) DMX_K2(1);
  else if (per <= 2) DMX_K2(2);
  else if (per <= 4) DMX_K2(4);
  else if (per <= 8) DMX_K2(8);
  else if (per <= 16) DMX_K2(16);
  else if (per <= 33) DMX_K2(33);
  else if (per <= 65) DMX_K2(65);
  else DMX_K2(33);                                // slabs of 33 * 256 accumulators
#undef DMX_K2
  return DMX_OK;
}

template <bool FIXUP>
int launch_doublet_generic_w(dmx_engine* e) {
  return e->nrd_width == 1 ? launch_doublet_generic<uint8_t, FIXUP>(e)
                           : (e->nrd_width == 2 ? launch_doublet_generic<uint16_t, FIXUP>(e) : launch_doublet_generic<uint32_t, FIXUP>(e));
}

// The A = 2 kernel with its fix-up pass; other alpha grids (or V > 64) take the generic kernel.
// FAST's soft-field kernels take their phase-2 terms through dmx_log2_lite, whose dropped r^5/5 term is at most 5.7e-15 per term with the sign of r:
// unbiased over varied inputs, but a barcode whose terms cluster on ONE value (a PL field repeats a handful of triples) can collect it linearly — the worst
// case is 6.7e-15 x (covered SNPs) with the result's own rounding (measured at the bin edges, tests/test_dmx_log.py), which reaches FAST's 1e-9 contract at
// 1.5e5.  Barcodes deeper than 130 000 covered SNPs run the STRICT kernels (bit-exact,
// inside FAST's contract); nothing in BASELINE.json comes near (cfg3: 5e4, cfg5: 1e4 covered SNPs per barcode; cfg4's GT classes take no per-term log).
constexpr int64_t kLiteLogMaxPairs = 130000;

int launch_doublet(dmx_engine* e) {
  const int32_t B = e->pv.B, V = e->V, A = e->A;
  e->k2_sym = false;
  const bool fast_soft = e->mode == DMX_MODE_FAST && (e->max_cell_pairs <= kLiteLogMaxPairs || e->knob("DMX_LITE_LOG_ANY_DEPTH"));
  const bool force_generic = e->knob("DMX_K2_GENERIC") != nullptr;      // kernel experiments only
  const bool use_cls = e->n_classes > 0 && !e->knob("DMX_NO_CLASSES");
  // j-slabs of a kernel that owns JS = tpc / ceil(V / nk) rows of the grid per workgroup (blockIdx.y)
  auto slabs_of = [&](int tpc, int nk) { const int kb = (V + nk - 1) / nk, js = tpc / kb; return (unsigned)((V + js - 1) / js); };
  if (A >= 3 && A <= 8 && use_cls && V <= 1024 && !force_generic) {
    // GT inputs, longer alpha grids: the class kernel with AP alphas per pair.  One cell per workgroup (the class table is
    // 4 x 4 x AP doubles per pair: 16-32 KB a tile); the k-block width follows the panel.
    const int AP = A <= 4 ? 4 : 8;
    const int VS = (V + 15) & ~15;
    size_t cb = (size_t)32 * AP * 9 * 8 + (size_t)32 * 16 * AP * 8 + (size_t)AP * 34 * 8 + 32 * (4 + 4 + 8) + (size_t)32 * 12 * 4 + (size_t)32 * VS;
    cb = (cb + 15) & ~(size_t)15;
    HIP_TRY(hipMemsetAsync(e->d_flag_base, 0, (size_t)B + kFlagHead, e->stream));
#define DMX_K2CN(NK, APP)                                                                                              \
  do {                                                                                                                 \
    if (cb > 60 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_doublet_clsn<256, NK, APP>),       \
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)cb));              \
    DMX_LAUNCH(k2_fn, (k_doublet_clsn<256, NK, APP>), dim3((unsigned)B, slabs_of(256, NK)), dim3(kThreads), cb, e->stream, \
                       e->pv, e->nrd_width, e->d_rows, e->d_ids, e->d_gp0, e->d_lut, e->d_alpha, e->d_sched, V, A, VS,   \
                       e->d_grid, e->d_l00, e->d_flag());                                                                  \
  } while (0)
    if (AP == 4) { if (V <= 16) DMX_K2CN(1, 4); else if (V <= 32) DMX_K2CN(4, 4); else DMX_K2CN(8, 4); }
    else         { if (V <= 16) DMX_K2CN(1, 8); else DMX_K2CN(4, 8); }
#undef DMX_K2CN
    HIP_TRY(hipGetLastError());
    return launch_doublet_generic_w<true>(e);
  }
  if (fast_soft && !use_cls && A >= 2 && A <= 8 && V <= 128 && e->alpha[0] == 0.0 && !(A == 2 && e->alpha[1] == 0.5) &&
      !force_generic && !e->knob("DMX_NO_ANF")) {
    // FAST, soft fields, any alpha grid that starts with 0 (the default grid {0, 0.5} has k_doublet_sym): the printed entries only,
    // bilinear form
    const int AP = A <= 2 ? 2 : (A <= 4 ? 4 : 8);
    const int GS = (V * 3 + 3) & ~3;
    HIP_TRY(hipMemsetAsync(e->d_flag_base, 0, (size_t)B + kFlagHead, e->stream));
    const dim3 block(kThreads);
#define DMX_K2NF_(TPC, NK, APP, VUS, SUBP, MINW, CHK)                                                                  \
  do {                                                                                                                 \
    const int NU = (A - 1) * 3 * VUS + 4;                                                                              \
    const size_t cell_bytes = (size_t)32 * APP * 9 * 8 + (size_t)32 * GS * 4 + (size_t)APP * 34 * 8 + 32 * (4 + 4 + 8) +  \
                              (size_t)SUBP * NU * 8 + (size_t)TPC * 8;                                                 \
    const size_t lds = cell_bytes * (kThreads / TPC);                                                                  \
    if (lds > 60 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_doublet_anf<TPC, NK, APP, VUS, SUBP, MINW, CHK>),  \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));            \
    DMX_LAUNCH(k2_fn, (k_doublet_anf<TPC, NK, APP, VUS, SUBP, MINW, CHK>), dim3((unsigned)((B + (kThreads / TPC) - 1) / (kThreads / TPC)), slabs_of(TPC, NK)), \
                       block, lds, e->stream, e->pv, e->nrd_width, e->d_g, e->d_gp0, e->d_lut,                            \
                       e->d_alpha, e->d_sched, V, A, GS, e->d_grid, e->d_l00, e->d_flag());                                \
  } while (0)
#define DMX_K2NF(TPC, NK, APP, VUS, SUBP, MINW) do { if (e->geno_safe) DMX_K2NF_(TPC, NK, APP, VUS, SUBP, MINW, false); else DMX_K2NF_(TPC, NK, APP, VUS, SUBP, MINW, true); } while (0)
    // u rows: V entries plus the slack a k-block may read past the panel's end (NK - 1), even; pairs per sub-tile by the LDS they need
    // (one barcode per workgroup throughout: the narrow-panel forms with four barcodes per workgroup need ~86 KB of LDS, i.e. one
    //  workgroup per CU; sub-tiles of 8 pairs and 3 wavefronts per SIMD measured 529 -> 418 ms at V = 32, A = 3, 4 000 barcodes)
    if (AP == 2) {
      if (V <= 16) DMX_K2NF(256, 1, 2, 16, 8, 3); else if (V <= 32) DMX_K2NF(256, 4, 2, 36, 8, 3);
      else if (V <= 64) DMX_K2NF(256, 8, 2, 72, 4, 2); else DMX_K2NF(256, 8, 2, 136, 2, 2);
    } else if (AP == 4) {
      if (V <= 16) DMX_K2NF(256, 1, 4, 16, 8, 3); else if (V <= 32) DMX_K2NF(256, 4, 4, 36, 8, 3);
      else if (V <= 64) DMX_K2NF(256, 8, 4, 72, 4, 2); else DMX_K2NF(256, 8, 4, 136, 2, 2);
    } else {
      if (V <= 16) DMX_K2NF(256, 1, 8, 16, 8, 2); else if (V <= 64) DMX_K2NF(256, 4, 8, 68, 2, 2);
      else DMX_K2NF(256, 4, 8, 132, 1, 2);
    }
#undef DMX_K2NF_
#undef DMX_K2NF
    HIP_TRY(hipGetLastError());
    return launch_doublet_generic_w<true>(e);
  }
  if (A >= 3 && A <= 8 && V <= (A <= 4 ? kAnMaxV4 : kAnMaxV8) && !force_generic) {
    // longer alpha grids: the A = 2 kernel's structure with AP alphas per pair (beyond ~130 samples with more than 64 KB of LDS, as k_doublet_a2)
    const int AP = A <= 4 ? 4 : 8;
    const int GS = (V * 3 + 3) & ~3;
    const size_t cell_bytes = (size_t)32 * AP * 9 * 8 + (size_t)32 * GS * 4 + (size_t)AP * 34 * 8 + 32 * (4 + 4 + 8);
    HIP_TRY(hipMemsetAsync(e->d_flag_base, 0, (size_t)B + kFlagHead, e->stream));
    const dim3 block(kThreads);
    // gfx950 lets one workgroup use all 160 KB of a CU's LDS; above the traditional 64 KB the limit is raised explicitly
#define DMX_K2N(TPC, NK, APP)                                                                                          \
  do {                                                                                                                 \
    const size_t lds = cell_bytes * (kThreads / TPC);                                                                  \
    if (lds > 60 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_doublet_an<TPC, NK, APP>),        \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));            \
    DMX_LAUNCH(k2_fn, (k_doublet_an<TPC, NK, APP>), dim3((unsigned)((B + (kThreads / TPC) - 1) / (kThreads / TPC)), slabs_of(TPC, NK)), \
                       block, lds, e->stream, e->pv, e->nrd_width, e->d_g, e->d_gp0, e->d_lut,                            \
                       e->d_alpha, e->d_sched, V, A, GS, e->d_grid, e->d_l00, e->d_flag());                                \
  } while (0)
    if (AP == 4) {
      if (V <= 8) DMX_K2N(64, 1, 4);
      else if (V <= 16) DMX_K2N(64, 4, 4);
      else if (V <= 32) DMX_K2N(256, 4, 4);
      else DMX_K2N(256, 8, 4);
    } else {
      if (V <= 8) DMX_K2N(64, 1, 8);
      else if (V <= 16) DMX_K2N(64, 4, 8);
      else DMX_K2N(256, 4, 8);
    }
#undef DMX_K2N
    HIP_TRY(hipGetLastError());
    return launch_doublet_generic_w<true>(e);
  }
  // wide panels: the class kernel's LDS grows by 32 bytes per sample, the general A = 2 kernel's by 384 (64 KB at V = 128)
  // (FAST on the default grid reaches 512 soft-field samples: k_doublet_sym's slabs keep their LDS flat in V)
  const bool sym_wide = fast_soft && !use_cls && A == 2 && e->alpha[0] == 0.0 && e->alpha[1] == 0.5 && V > 128 && V <= 512 &&
                        !e->knob("DMX_NO_SYM") && !e->knob("DMX_NO_SYM_WIDE");
  // (round 4: the general A = 2 kernel itself runs up to kA2MaxV = 1024 samples — one workgroup may use all 160 KB of a gfx950 CU's LDS, and the
  // tile shortens from 32 to 16 or 8 pairs as the rows grow; beyond, the generic kernel)
  if (A != 2 || force_generic || (V > (use_cls ? 1024 : kA2MaxV) && !sym_wide)) {
    HIP_TRY(hipMemsetAsync(e->d_flag_base, 0, (size_t)B + kFlagHead, e->stream));
    if (int rc = launch_doublet_generic_w<false>(e)) return rc;
    HIP_TRY(hipGetLastError());
    return launch_doublet_generic_w<true>(e);
  }
  if (use_cls && e->mode == DMX_MODE_FAST && e->alpha[0] == 0.0 && e->alpha[1] == 0.5 && V <= 64 && !e->knob("DMX_NO_SYM")) {
    if (V > 32 && !e->knob("DMX_FAST_NO_PROD")) {
      // 33..64 samples: the producer / consumer kernel over the printed entries (round 4; k_doublet_clsym<33,2> ran 2 wavefronts per SIMD)
      HIP_TRY(hipMemsetAsync(e->d_flag_base, 0, (size_t)B + kFlagHead, e->stream));
      const size_t lds = (size_t)2 * 32 * 32 * 8 + (size_t)2 * 32 * 64 + (size_t)32 * 18 * 8 + 2 * 34 * 8 + 2 * 32 * (8 + 4 + 4) +
                         (size_t)32 * 12 * 4;
      DMX_LAUNCH(k2_fn, (k_doublet_clsp<3, true>), dim3((unsigned)B), dim3(kThreads), lds, e->stream, e->pv, e->nrd_width, e->d_rows, e->d_ids,
                         e->d_gp0, e->d_lut, e->d_alpha, e->d_sched, V, 0, e->d_grid, e->d_l00, e->d_flag());
      HIP_TRY(hipGetLastError());
      return launch_doublet_generic_w<true>(e);
    }
    // GT inputs, default grid {0, 0.5}, FAST: class table + the printed entries only, one wavefront per barcode
    const int D = V / 2 + 1, Q = 64 / V;
    // offsets per lane NED and slabs NS with Q * NED * NS >= D: as few slabs as 17 accumulators per lane allow (more do not fit
    // the register file beside the kernel's invariants at 3 wavefronts per SIMD), then the smallest NED
    int NS = (D + Q * 17 - 1) / (Q * 17);
    // ... except that a panel that would need two slabs of 17 runs as ONE slab of up to 33 at 2 wavefronts per SIMD (212
    // registers, no spills): every slab repeats phase 1 and the class table, which is two thirds of a 17-offset slab's time
    // (cfg4, 6 144 barcodes: 267 ms against 302 ms)
    if (NS == 2 && (D + Q - 1) / Q <= 33) NS = 1;
    if (const char* env = e->knob("DMX_CLSYM_NED")) NS = (D + Q * atoi(env) - 1) / (Q * atoi(env));   // kernel experiments only
    const int need = (D + Q * NS - 1) / (Q * NS);
    HIP_TRY(hipMemsetAsync(e->d_flag_base, 0, (size_t)B + kFlagHead, e->stream));
    constexpr size_t cb = ((size_t)8 * 32 * 8 + 32 * 6 * 8 + 32 * 4 * 8 + 2 * 34 * 8 + 32 * 16 + 32 * 12 * 4 + 32 * 10 * 4 + 63) & ~(size_t)63;
    static_assert(cb % 64 == 0, "a barcode's LDS block keeps its class table 64-byte aligned (k_doublet_clsym ORs the class offset in)");
#define DMX_K2CS(NED, MINW)                                                                                            \
  DMX_LAUNCH(k2_fn, (k_doublet_clsym<NED, MINW>), dim3((unsigned)((B + 3) / 4), (unsigned)NS), dim3(kThreads), cb * 4, e->stream, e->pv, \
                     e->nrd_width, e->d_rows, e->d_idd, e->nwd2, e->d_gp0, e->d_lut, e->d_sched, V, e->d_grid, e->d_l00, e->d_flag())
    if (need <= 1) DMX_K2CS(1, 4); else if (need <= 2) DMX_K2CS(2, 4); else if (need <= 3) DMX_K2CS(3, 4); else if (need <= 5) DMX_K2CS(5, 4);
    else if (need <= 7) DMX_K2CS(7, 3); else if (need <= 9) DMX_K2CS(9, 3); else if (need <= 11) DMX_K2CS(11, 3);
    else if (need <= 13) DMX_K2CS(13, 3); else if (need <= 15) DMX_K2CS(15, 3); else if (need <= 17) DMX_K2CS(17, 3);
    else if (need <= 25) DMX_K2CS(25, 2); else DMX_K2CS(33, 2);   // one slab, 2 wavefronts per SIMD
#undef DMX_K2CS
    HIP_TRY(hipGetLastError());
    return launch_doublet_generic_w<true>(e);
  }
  if (use_cls) {
    const int VS = (V <= 32) ? ((V + 3) & ~3) : ((V + 15) & ~15);   // id row stride: a whole number of k-blocks
    size_t cb = (size_t)32 * 18 * 8 + (size_t)32 * 32 * 8 + 2 * 34 * 8 + 32 * (4 + 4 + 8) + (size_t)32 * 12 * 4 + (size_t)32 * VS;
    if (V > 32) cb += 32 * 16;                      // the pipelined form's second header buffer
    cb = (cb + 15) & ~(size_t)15;
    HIP_TRY(hipMemsetAsync(e->d_flag_base, 0, (size_t)B + kFlagHead, e->stream));
    const dim3 blk(kThreads);
#define DMX_K2C(TPC, NK, ...)                                                                                        \
  DMX_LAUNCH(k2_fn, (k_doublet_cls<TPC, NK, ##__VA_ARGS__>), dim3((unsigned)((B + (kThreads / TPC) - 1) / (kThreads / TPC)), slabs_of(TPC, NK)), blk,   \
                     cb * (kThreads / TPC), e->stream, e->pv, e->nrd_width, e->d_rows, e->d_ids, e->d_gp0, e->d_lut,   \
                     e->d_alpha, e->d_sched, V, VS, e->d_grid, e->d_l00, e->d_flag())
    if (V <= 8) DMX_K2C(64, 1);
    else if (V <= 16) DMX_K2C(64, 4);
    else if (V <= 32) DMX_K2C(256, 4);
    else if (e->knob("DMX_CLS_MINW3")) DMX_K2C(256, 16, 3);    // kernel experiments only (36 spills: slower)
    else if (e->knob("DMX_CLS_NK8")) { if (atoi(e->knob("DMX_CLS_NK8")) == 3) DMX_K2C(256, 8, 3); else DMX_K2C(256, 8); }
    else if (V <= 64 && !e->knob("DMX_CLS_NO_PROD") && !e->knob("DMX_CLS_NO_UJ")) {
      // producer / consumer form (round 4): one barrier per tile, wavefront 0 builds the next tile's class table, 3 wavefronts per SIMD
      const size_t lds = (size_t)2 * 32 * 32 * 8 + (size_t)2 * 32 * 64 + (size_t)32 * 18 * 8 + 2 * 34 * 8 + 2 * 32 * (8 + 4 + 4) +
                         (size_t)32 * 12 * 4;
      DMX_LAUNCH(k2_fn, (k_doublet_clsp<3>), dim3((unsigned)B), dim3(kThreads), lds, e->stream, e->pv, e->nrd_width, e->d_rows, e->d_ids, e->d_gp0,
                         e->d_lut, e->d_alpha, e->d_sched, V, VS, e->d_grid, e->d_l00, e->d_flag());
    }
    else if (V <= 64 && !e->knob("DMX_CLS_NO_UJ")) DMX_K2C(256, 16, 2, true);   // uniform-j form (a wavefront's 16 samples j share their class per pair)
    else DMX_K2C(256, 16);
#undef DMX_K2C
    HIP_TRY(hipGetLastError());
    return launch_doublet_generic_w<true>(e);
  }
  const int GS = (V * 3 + 3) & ~3;               // LDS row stride of a genotype row (floats), 16-byte multiple
  const size_t cell_bytes = (size_t)32 * 18 * 8 + (size_t)32 * GS * 4 + 2 * 34 * 8 + 32 * (4 + 4 + 8);
  HIP_TRY(hipMemsetAsync(e->d_flag_base, 0, (size_t)B + kFlagHead, e->stream));
  const dim3 block(kThreads);
  // k_doublet_a2's phase 1 on the default grid {0, 0.5}: finished values of pairs of up to three tabled reads from the table (round 6; shallow pileups only,
  // ensure_finals; DMX_A2_NO_FINALS=1: the read loop everywhere) — other grids have other mixing weights and keep the loop
  const double* pfin_a2 = nullptr;
  const bool pfin_a2_grid = A == 2 && e->alpha[0] == 0.0 && e->alpha[1] == 0.5;
  if (pfin_a2_grid && !e->knob("DMX_A2_NO_FINALS")) if (int rc = ensure_finals(e, &pfin_a2)) return rc;
  const double* pseed_a2 = nullptr;              // ... and the tiles that walk the loop walk it in the five-value form from the seed table (DMX_A2_NO_SEEDS=1: the nine-value loop)
  if (pfin_a2_grid && !e->knob("DMX_A2_NO_SEEDS")) if (int rc = ensure_seeds(e, &pseed_a2)) return rc;
#define DMX_K2A(TPC, NK)                                                                                             \
  do {                                                                                                                \
    if (e->geno_safe)                                                                                                 \
      DMX_LAUNCH(k2_fn, (k_doublet_a2<TPC, NK, 1, false, false>), dim3((unsigned)((B + (kThreads / TPC) - 1) / (kThreads / TPC)), slabs_of(TPC, NK)), block,  \
                         cell_bytes * (kThreads / TPC), e->stream, e->pv, e->nrd_width, e->d_g, e->d_gp0, e->d_lut,    \
                         e->d_alpha, e->d_sched, V, GS, e->d_grid, e->d_l00, e->d_flag(), pfin_a2, pseed_a2);                               \
    else                                                                                                              \
  DMX_LAUNCH(k2_fn, (k_doublet_a2<TPC, NK>), dim3((unsigned)((B + (kThreads / TPC) - 1) / (kThreads / TPC)), slabs_of(TPC, NK)), block,  \
                     cell_bytes * (kThreads / TPC), e->stream, e->pv, e->nrd_width, e->d_g, e->d_gp0, e->d_lut,        \
                     e->d_alpha, e->d_sched, V, GS, e->d_grid, e->d_l00, e->d_flag(), pfin_a2, pseed_a2);                                   \
  } while (0)
  if (fast_soft && e->alpha[0] == 0.0 && e->alpha[1] == 0.5 && (V <= 128 || sym_wide) && !e->knob("DMX_NO_SYM")) {
    // demuxlet's default grid {0, 0.5}: only the printed entries (singlet column + one evaluation per unordered pair)
    const double* pfin = nullptr;                 // phase 1's finished values of pairs of up to three tabled reads (DMX_SYM_NO_FINALS=1: the read loop everywhere)
    if (!e->knob("DMX_SYM_NO_FINALS")) if (int rc = ensure_finals(e, &pfin)) return rc;
    const double* pseed = nullptr;                // the state after a pair's first one or two reads (DMX_SYM_NO_SEEDS=1: the loop from its start)
    if (!e->knob("DMX_SYM_NO_SEEDS")) if (int rc = ensure_seeds(e, &pseed)) return rc;
#define DMX_K2S(TPC, VMAX, SUB, FIX)                                                                                  \
  do { e->k2_sym = true;                                                                                                                \
    constexpr int GSS_ = (3 * VMAX + 3) & ~3, VUS_ = (VMAX + 2) & ~1, TP_ = TPC >= 64 ? 32 : TPC / 2;                   \
    constexpr size_t cb_ = (size_t)TP_ * 6 * 8 + TP_ * 4 * 8 + 2 * (TP_ + 2) * 8 + TP_ * 16 + (size_t)(TPC == 32 ? 3 : (TPC >= 32 ? 2 : 1)) * SUB * GSS_ * 4 + (size_t)SUB * 3 * VUS_ * 8; \
    const size_t lds = cb_ * (kThreads / TPC);                                                                         \
    if (lds > 60 * 1024) {                                                                                             \
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_doublet_sym<TPC, VMAX, SUB, FIX>),                  \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                              \
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_doublet_sym<TPC, VMAX, SUB, FIX, 3, 0, false>),     \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                              \
    }                                                                                                                  \
    if (e->geno_safe)                                                                                                  \
      DMX_LAUNCH(k2_fn, (k_doublet_sym<TPC, VMAX, SUB, FIX, 3, 0, false>), dim3((unsigned)((B + (kThreads / TPC) - 1) / (kThreads / TPC))), \
                         block, lds, e->stream, e->pv, e->nrd_width, e->d_g, e->d_gp0, e->d_lut, e->d_sched, V | sym_flags,         \
                         e->d_grid, e->d_l00, e->d_flag(), pfin, pseed);                                                              \
    else                                                                                                               \
    DMX_LAUNCH(k2_fn, (k_doublet_sym<TPC, VMAX, SUB, FIX>), dim3((unsigned)((B + (kThreads / TPC) - 1) / (kThreads / TPC))), \
                       block, lds, e->stream, e->pv, e->nrd_width, e->d_g, e->d_gp0, e->d_lut, e->d_sched, V | sym_flags,           \
                       e->d_grid, e->d_l00, e->d_flag(), pfin, pseed);                                                                \
  } while (0)
#define DMX_K2SV(TPC, VMAX, SUB, FIX, MINW)                                                                            \
  do { e->k2_sym = true;                                                                                                                \
    constexpr int GSS_ = (3 * VMAX + 3) & ~3, VUS_ = (VMAX + 2) & ~1, TP_ = TPC >= 64 ? 32 : TPC / 2;                   \
    constexpr size_t cb_ = (size_t)TP_ * 6 * 8 + TP_ * 4 * 8 + 2 * (TP_ + 2) * 8 + TP_ * 16 + (size_t)(TPC == 32 ? 3 : (TPC >= 32 ? 2 : 1)) * SUB * GSS_ * 4 + (size_t)SUB * 3 * VUS_ * 8; \
    const size_t lds = cb_ * (kThreads / TPC);                                                                         \
    if (lds > 60 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_doublet_sym<TPC, VMAX, SUB, FIX, MINW>), \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));          \
    DMX_LAUNCH(k2_fn, (k_doublet_sym<TPC, VMAX, SUB, FIX, MINW>), dim3((unsigned)((B + (kThreads / TPC) - 1) / (kThreads / TPC))), \
                       block, lds, e->stream, e->pv, e->nrd_width, e->d_g, e->d_gp0, e->d_lut, e->d_sched, V | sym_flags,           \
                       e->d_grid, e->d_l00, e->d_flag(), pfin, pseed);                                                                \
  } while (0)
    const int32_t sym_flags = (e->knob("DMX_SYM_NO_DMA") ? (1 << 16) : 0) | (e->knob("DMX_SYM_ABLATE_P1") ? (1 << 17) : 0) |
                              (e->knob("DMX_SYM_ABLATE_P2") ? (1 << 18) : 0) | (e->knob("DMX_SYM_ABLATE_U") ? (1 << 19) : 0) |
                              (e->knob("DMX_SYM_ABLATE_RD") ? (1 << 20) : 0) | (e->knob("DMX_SYM_ABLATE_00") ? (1 << 21) : 0) | (e->knob("DMX_SYM_NO_PRODUCT") ? (1 << 22) : 0) |
                              (e->knob("DMX_SYM_NO_PIPE") ? (1 << 23) : 0) | (e->knob("DMX_SYM_WAIT_ALL") ? (1 << 24) : 0);       // kernel experiments only (the ABLATE bits do something in -DDMX_SYM_ABLATIONS=1 builds only)
    const bool wide_cells = e->knob("DMX_SYM_ONE_CELL_PER_WAVE") != nullptr;   // kernel experiments only
    if (V <= 8 && !wide_cells) { if (16 % V == 0) DMX_K2S(16, 8, 4, true); else DMX_K2S(16, 8, 4, false); }        // four barcodes per wavefront
    else if (V <= 16 && !wide_cells) { if (V == 16) DMX_K2S(32, 16, 4, true); else DMX_K2S(32, 16, 4, false); }   // two
    else if (V <= 8) { if (64 % V == 0) DMX_K2S(64, 8, 4, true); else DMX_K2S(64, 8, 4, false); }
    else if (V <= 17) { if (V == 16) DMX_K2S(64, 17, 4, true); else DMX_K2S(64, 17, 4, false); }
    else if (V <= 23) DMX_K2S(64, 23, 4, false);
    else if (V <= 27) DMX_K2S(64, 27, 4, false);
    else if (V <= 32) {
      if (V == 32) {
        const int var = e->knob("DMX_SYM_VARIANT") ? atoi(e->knob("DMX_SYM_VARIANT")) : 0;      // kernel experiments only
        if (var == 1) DMX_K2SV(64, 32, 2, true, 4); else if (var == 2) DMX_K2SV(64, 32, 4, true, 4); else if (var == 3) DMX_K2SV(64, 32, 8, true, 3);
        else if (var == 4) DMX_K2SV(64, 32, 2, true, 3); else if (var == 5) DMX_K2SV(64, 32, 8, true, 2); else DMX_K2S(64, 32, 4, true);
      } else DMX_K2S(64, 32, 4, false);
    }
    else if (V <= 48) DMX_K2S(256, 48, 8, false);
    else if (V <= 64) { if (V == 64) DMX_K2S(256, 64, 8, true); else DMX_K2S(256, 64, 8, false); }
    else {
      // 64 < V <= 512: the entry list (V (V/2 + 1) + V, up to 132 096) in slabs of 9 entries per lane
      const unsigned ns = (unsigned)((V * (V / 2 + 1) + V + 256 * 9 - 1) / (256 * 9));
#define DMX_K2SS(VMAX, SUB, FIX)                                                                                       \
  do { e->k2_sym = true;                                                                                                                \
    constexpr int GSS_ = (3 * VMAX + 3) & ~3, VUS_ = (VMAX + 2) & ~1;                                                  \
    constexpr size_t cb_ = (size_t)32 * 6 * 8 + 32 * 4 * 8 + 2 * 34 * 8 + 32 * 16 + (size_t)2 * SUB * GSS_ * 4 + (size_t)SUB * 3 * VUS_ * 8; \
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_doublet_sym<256, VMAX, SUB, FIX, 3, 9>),              \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)cb_));                               \
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_doublet_sym<256, VMAX, SUB, FIX, 3, 9, false>),       \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)cb_));                               \
    if (e->geno_safe)                                                                                                  \
      DMX_LAUNCH(k2_fn, (k_doublet_sym<256, VMAX, SUB, FIX, 3, 9, false>), dim3((unsigned)B, ns), block, cb_, e->stream, e->pv, \
                         e->nrd_width, e->d_g, e->d_gp0, e->d_lut, e->d_sched, V | sym_flags, e->d_grid, e->d_l00, e->d_flag(), pfin, pseed);      \
    else                                                                                                               \
    DMX_LAUNCH(k2_fn, (k_doublet_sym<256, VMAX, SUB, FIX, 3, 9>), dim3((unsigned)B, ns), block, cb_, e->stream, e->pv, \
                       e->nrd_width, e->d_g, e->d_gp0, e->d_lut, e->d_sched, V | sym_flags, e->d_grid, e->d_l00, e->d_flag(), pfin, pseed);        \
  } while (0)
      if (V <= 96) DMX_K2SS(96, 8, false); else if (V == 128) DMX_K2SS(128, 8, true); else if (V < 128) DMX_K2SS(128, 8, false);
      else if (V <= 192) DMX_K2SS(192, 4, false); else if (V <= 256) DMX_K2SS(256, 4, false);        // (sub-tiles of 4 pairs: 40 / 53 KB of LDS per workgroup)
      else if (V <= 384) DMX_K2SS(384, 2, false); else DMX_K2SS(512, 2, false);        // (round 4: 257..512 samples, sub-tiles of 2 pairs: 40 / 53 KB)
#undef DMX_K2SS
    }
#undef DMX_K2SV
#undef DMX_K2S
    HIP_TRY(hipGetLastError());
    return launch_doublet_generic_w<true>(e);
  }
  if (fast_soft && V <= 128) {     // (wider panels that are not k_doublet_sym's run the STRICT kernel below: bit-exact, inside FAST's contract)
    // one-cell-per-workgroup panels share u through LDS (cfg3 1.33x); one-wavefront cells (V <= 16) form it in registers
    const size_t fast_bytes = cell_bytes + (V > 16 ? (size_t)8 * 2 * V * 32 : 0);
#define DMX_K2F(TPC, NK)                                                                                             \
  do {                                                                                                               \
    const size_t lds = fast_bytes * (kThreads / TPC);                                                                \
    if (lds > 60 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_doublet_a2f<TPC, NK>),          \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));          \
    DMX_LAUNCH(k2_fn, (k_doublet_a2f<TPC, NK>), dim3((unsigned)((B + (kThreads / TPC) - 1) / (kThreads / TPC)), slabs_of(TPC, NK)), \
                       block, lds, e->stream, e->pv, e->nrd_width, e->d_g, e->d_gp0, e->d_lut, e->d_alpha, e->d_sched, V, GS,           \
                       e->d_grid, e->d_l00, e->d_flag());                                                              \
  } while (0)
    if (V <= 8) DMX_K2F(64, 1);
    else if (V <= 16) DMX_K2F(64, 4);
    else if (V <= 32) DMX_K2F(256, 4);
    else DMX_K2F(256, 16);
#undef DMX_K2F
    HIP_TRY(hipGetLastError());
    return launch_doublet_generic_w<true>(e);
  }
  if (V == 32 && pfin_a2_grid && e->geno_safe && !e->knob("DMX_A2_SYM") && !e->knob("DMX_A2_NO_SYMU") && !e->knob("DMX_A2_NO_GD") && !e->knob("DMX_A2_MINW1")) {
    // 32 soft-field samples on the default grid (cfg3, the headline): k_doublet_a2's kernel over UNORDERED pairs — a thread owns [j][k] and [k][j] and forms
    // the products they share once — and the 64 diagonal accumulators of a barcode on one wavefront behind it (DMX_A2_NO_SYMU=1: k_doublet_a2)
    // dense pileups (pair p of every barcode is SNP p, every barcode has the same pair count): two barcodes per workgroup share the products g_j[l] g_k[m] of
    // a unit, one slab of the unordered pairs per workgroup (DMX_A2U_ONE_BARCODE=1: k_doublet_a2u)
    const size_t cbd = (size_t)32 * 18 * 8 + (size_t)32 * GS * 8 + 2 * 34 * 8 + 32 * (4 + 4 + 8);
    const bool two_barcodes = e->pv.pair_snp == nullptr && !e->knob("DMX_A2U_ONE_BARCODE");
    const bool diag16 = two_barcodes && !e->knob("DMX_A2U2_NO_DIAG") && !e->knob("DMX_A2U_DIAG_WAVE");   // the entries [j][j], j = 16..31, in k_doublet_a2u2's idle slots
    if (diag16 && e->knob("DMX_A2U_MIRROR_FALLBACK"))   // tests only: the two-barcode kernel with every mirrored log on its slow path
      DMX_LAUNCH(k2_fn, (k_doublet_a2u<k_doublet_a2u2_mirror_fallback>), dim3((unsigned)((B + 1) / 2), 2), block, 0, e->stream, e->pv, e->nrd_width, e->d_g,
                         e->d_gp0, e->d_lut, e->d_alpha, e->d_sched, e->d_grid, e->d_l00, e->d_flag(), pfin_a2, pseed_a2);
    else if (diag16)
      DMX_LAUNCH(k2_fn, (k_doublet_a2u<k_doublet_a2u2>), dim3((unsigned)((B + 1) / 2), 2), block, 0, e->stream, e->pv, e->nrd_width, e->d_g,
                         e->d_gp0, e->d_lut, e->d_alpha, e->d_sched, e->d_grid, e->d_l00, e->d_flag(), pfin_a2, pseed_a2);
    else if (two_barcodes)
      DMX_LAUNCH(k2_fn, (k_doublet_a2u<k_doublet_a2u2_whole_diag_behind>), dim3((unsigned)((B + 1) / 2), 2), block, 0, e->stream, e->pv, e->nrd_width, e->d_g,
                         e->d_gp0, e->d_lut, e->d_alpha, e->d_sched, e->d_grid, e->d_l00, e->d_flag(), pfin_a2, pseed_a2);
    else
    DMX_LAUNCH(k2_fn, (k_doublet_a2u<4>), dim3((unsigned)B, 1), block, cbd, e->stream, e->pv, e->nrd_width, e->d_g,
                       e->d_gp0, e->d_lut, e->d_alpha, e->d_sched, V, GS, e->d_grid, e->d_l00, e->d_flag(), pfin_a2, pseed_a2);
    if (diag16)
      hipLaunchKernelGGL((k_doublet_diag_lo<5>), dim3((unsigned)((B + 15) / 16)), block, 0, e->stream, e->pv, e->nrd_width, e->d_g, e->d_lut, e->d_sched, e->d_grid, pfin_a2, pseed_a2);
    else if (e->knob("DMX_A2U_DIAG_WAVE"))             // kernel experiments only: the diagonal on one wavefront per barcode (the first form)
      hipLaunchKernelGGL((k_doublet_a2s<4, 4, 0>), dim3((unsigned)((B + 3) / 4), 1), block, 0, e->stream, e->pv, e->nrd_width, e->d_g, e->d_gp0, e->d_lut, e->d_sched,
                         e->d_grid, e->d_l00, pfin_a2);
    else
      hipLaunchKernelGGL((k_doublet_diag<5>), dim3((unsigned)((B + 7) / 8)), block, 0, e->stream, e->pv, e->nrd_width, e->d_g, e->d_lut, e->d_sched, e->d_grid, pfin_a2, pseed_a2);
  }
  else if (V == 32 && pfin_a2_grid && e->geno_safe && e->knob("DMX_A2_SYM")) {
    // 32 soft-field samples on the default grid (cfg3, the headline): symmetric ownership — one lane owns [j][k] and [k][j], their shared products once.
    // An EXPERIMENT (DMX_A2_SYM=1), bit-identical, 9 % fewer instructions (967 FP64 + 212 others against 1 040 + 260 per covered pair and barcode) and
    // about as fast: the 17 accumulators per lane do not fit four wavefronts per SIMD (128 registers: 18 spill accesses per pair in the loop, 3 139 ms),
    // and at three it runs alone 1 206 ms (sub-tiles of 8 pairs, DMX_A2S_SUB8=1: 1 177-1 191) against k_doublet_a2's 1 214-1 223 on the same boxes, the STEP
    // 1 229-1 235 against 1 237-1 250 — K1 beside it costs it more than it costs k_doublet_a2.  Not worth a second headline kernel.
    const dim3 grds((unsigned)((B + 3) / 4), 2);
    if (e->knob("DMX_A2S_SUB8"))                 // kernel experiments only
      DMX_LAUNCH(k2_fn, (k_doublet_a2s<8, 3>), grds, block, 0, e->stream, e->pv, e->nrd_width, e->d_g, e->d_gp0, e->d_lut, e->d_sched, e->d_grid, e->d_l00, pfin_a2);
    else if (!e->knob("DMX_A2S_MINW4"))          // (three wavefronts per SIMD unless the spilling four-wavefront form is asked for)
      DMX_LAUNCH(k2_fn, (k_doublet_a2s<4, 3>), grds, block, 0, e->stream, e->pv, e->nrd_width, e->d_g, e->d_gp0, e->d_lut, e->d_sched, e->d_grid, e->d_l00, pfin_a2);
    else
      DMX_LAUNCH(k2_fn, (k_doublet_a2s<4, 4>), grds, block, 0, e->stream, e->pv, e->nrd_width, e->d_g, e->d_gp0, e->d_lut, e->d_sched, e->d_grid, e->d_l00, pfin_a2);
  }
  else if (V == 16 && pfin_a2_grid && e->geno_safe && !e->knob("DMX_A2_NO_SYMU")) {
    // 16 soft-field samples on the default grid (cfg5): the same — unordered pairs on k_doublet_a2<64,4>'s kernel, the diagonal on 16 lanes per barcode behind it
    if (e->knob("DMX_A2U_MIRROR_FALLBACK"))            // tests only: every mirrored log on its slow path
      DMX_LAUNCH(k2_fn, (k_doublet_a2u16_mirror_fallback), dim3((unsigned)((B + 3) / 4), 1), block, cell_bytes * 4, e->stream, e->pv, e->nrd_width, e->d_g,
                         e->d_gp0, e->d_lut, e->d_alpha, e->d_sched, V, GS, e->d_grid, e->d_l00, e->d_flag(), pfin_a2, pseed_a2);
    else
    DMX_LAUNCH(k2_fn, (k_doublet_a2u16), dim3((unsigned)((B + 3) / 4), 1), block, cell_bytes * 4, e->stream, e->pv, e->nrd_width, e->d_g,
                       e->d_gp0, e->d_lut, e->d_alpha, e->d_sched, V, GS, e->d_grid, e->d_l00, e->d_flag(), pfin_a2, pseed_a2);
    hipLaunchKernelGGL((k_doublet_diag<5, 16>), dim3((unsigned)((B + 15) / 16)), block, 0, e->stream, e->pv, e->nrd_width, e->d_g, e->d_lut, e->d_sched, e->d_grid, pfin_a2, pseed_a2);
  }
  else if (V <= 8) DMX_K2A(64, 1);
  else if (V <= 16) DMX_K2A(64, 4);
  else if (V <= 32) {
    // 4 wavefronts per SIMD (128 VGPRs, a few spills outside the hot loop) measured 2.8 % faster than 3 (158 VGPRs) on cfg3
    if (!e->knob("DMX_A2_NO_GD") && !e->knob("DMX_A2_MINW1")) {   // rows widened to binary64 at staging: 1-2.5 % (cfg3, 5 000 barcodes: 741-753 vs 760 ms)
      const size_t cbd = (size_t)32 * 18 * 8 + (size_t)32 * GS * 8 + 2 * 34 * 8 + 32 * (4 + 4 + 8);
      if (e->geno_safe)
        DMX_LAUNCH(k2_fn, (k_doublet_a2<256, 4, 4, true, false>), dim3((unsigned)B, slabs_of(256, 4)), block, cbd, e->stream, e->pv, e->nrd_width, e->d_g,
                           e->d_gp0, e->d_lut, e->d_alpha, e->d_sched, V, GS, e->d_grid, e->d_l00, e->d_flag(), pfin_a2, pseed_a2);
      else
      DMX_LAUNCH(k2_fn, (k_doublet_a2<256, 4, 4, true>), dim3((unsigned)B, slabs_of(256, 4)), block, cbd, e->stream, e->pv, e->nrd_width, e->d_g,
                         e->d_gp0, e->d_lut, e->d_alpha, e->d_sched, V, GS, e->d_grid, e->d_l00, e->d_flag(), pfin_a2, pseed_a2);
    } else if (!e->knob("DMX_A2_MINW1"))
      DMX_LAUNCH(k2_fn, (k_doublet_a2<256, 4, 4>), dim3((unsigned)B, slabs_of(256, 4)), block, cell_bytes, e->stream, e->pv, e->nrd_width, e->d_g,
                         e->d_gp0, e->d_lut, e->d_alpha, e->d_sched, V, GS, e->d_grid, e->d_l00, e->d_flag(), pfin_a2, pseed_a2);
    else DMX_K2A(256, 4);
  }
  else if (V <= 128) DMX_K2A(256, 16);            // <= 55 KB of LDS
  else {
    // 129..1024 samples (round 4; the generic kernel before): the same kernel with the tile as long as leaves TWO workgroups per CU
    // (32 pairs up to 181 samples, 16 up to 377, 8 up to 770), else the longest that fits one workgroup's 160 KB; above 64 KB
    // the limit is raised explicitly.  2.2-3.6x the generic kernel's rate, bit-identical to it (tools/probe_wide_strict.py).
    auto bytes_of = [&](int tp) { return (size_t)tp * 18 * 8 + (size_t)tp * GS * 4 + 2 * (size_t)(tp + 2) * 8 + (size_t)tp * (4 + 4 + 8); };
    constexpr size_t kStatic = sizeof(double) * kTab2 + 2 * 18 * sizeof(double), kTwo = 80 * 1024, kOne = 160 * 1024;   // (the kernel's static LDS: s_tab, s_w)
    int tp = 0;
    for (int c : {32, 16, 8}) if (!tp && bytes_of(c) + kStatic <= kTwo) tp = c;
    for (int c : {32, 16, 8}) if (!tp && bytes_of(c) + kStatic <= kOne) tp = c;
    if (const char* env = e->knob("DMX_A2_TP")) { const int c = atoi(env); if ((c == 32 || c == 16 || c == 8) && bytes_of(c) + kStatic <= kOne) tp = c; }   // kernel experiments only
    if (!tp) return set_error(DMX_ERR_ARG, "run_doublet: V = %d exceeds k_doublet_a2's LDS budget", (int)V);
    const size_t lds = bytes_of(tp);
#define DMX_K2AW(TPP)                                                                                                 \
  do {                                                                                                                \
    if (e->geno_safe) {                                                                                               \
      if (lds > 60 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_doublet_a2<256, 16, 1, false, false, TPP>),  \
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));        \
      DMX_LAUNCH(k2_fn, (k_doublet_a2<256, 16, 1, false, false, TPP>), dim3((unsigned)B, slabs_of(256, 16)), block, lds, e->stream, e->pv,  \
                         e->nrd_width, e->d_g, e->d_gp0, e->d_lut, e->d_alpha, e->d_sched, V, GS, e->d_grid, e->d_l00, e->d_flag(), pfin_a2, pseed_a2);  \
    } else {                                                                                                          \
      if (lds > 60 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_doublet_a2<256, 16, 1, false, true, TPP>),   \
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));        \
      DMX_LAUNCH(k2_fn, (k_doublet_a2<256, 16, 1, false, true, TPP>), dim3((unsigned)B, slabs_of(256, 16)), block, lds, e->stream, e->pv,   \
                         e->nrd_width, e->d_g, e->d_gp0, e->d_lut, e->d_alpha, e->d_sched, V, GS, e->d_grid, e->d_l00, e->d_flag(), pfin_a2, pseed_a2);  \
    }                                                                                                                 \
  } while (0)
    if (tp == 32) DMX_K2AW(32); else if (tp == 16) DMX_K2AW(16); else DMX_K2AW(8);
#undef DMX_K2AW
  }
#undef DMX_K2A
  HIP_TRY(hipGetLastError());
  return launch_doublet_generic_w<true>(e);
}

}  // namespace

namespace {
int launch_certify(dmx_engine* e) {
  const int32_t B = e->pv.B;
  // sparse pileups over a matrix beyond the L2: one launch per SNP block (the table of the blocked K1 walk), state parked in between
  // — OFF by default: measured at cfg5 it cuts K3b's L2-side traffic (profiles/r04_certify_blocks.txt) but costs time (10.15 against 9.28 ms: the kernel is
  // bound by its own instruction stream, and 25 launches with their partial tiles cost more than the L2 hits save); DMX_CERTIFY_BLOCKS=1 turns it on,
  // and forced small blocks (DMX_K1_BLOCK_BYTES) always use it so that the tests cover the parked-state path
  const int64_t* blk = (e->pv.pair_snp && e->blk_n > 1 && (e->knob("DMX_CERTIFY_BLOCKS") || e->knob("DMX_K1_BLOCK_BYTES"))) ? e->d_blk : nullptr;
  const int bstride = (blk && e->knob("DMX_CERTIFY_BLOCK_STRIDE")) ? std::max(1, atoi(e->knob("DMX_CERTIFY_BLOCK_STRIDE"))) : 1;   // table blocks per launch
  const int n_launch = blk ? (e->blk_n + bstride - 1) / bstride : 1;
  double* park = nullptr;
  if (blk) {
    if (int rc = e->d_park.ensure(sizeof(double) * kPark * (size_t)std::max(B, 1))) return rc;
    park = e->d_park;
  }
  const float* gT = (!e->pv.pair_snp && e->have_gT && !e->knob("DMX_CERTIFY_NO_GT")) ? e->d_gT : nullptr;   // dense pileups: SNP-minor columns
#define DMX_K3B(MINW_, FIVE_, DENSE_)                                                                                  \
  for (int bi = 0; bi < n_launch; ++bi)                                                                                 \
    DMX_LAUNCH(k3b_fn, (k_certify<MINW_, FIVE_, DENSE_>), dim3((unsigned)((B + 3) / 4)), dim3(kThreads), 0, e->stream, e->pv, e->nrd_width, e->d_g, gT, \
                       e->d_lut, e->d_alpha, e->V, e->d_sum, blk, (bi * bstride) | (bstride << 16), e->blk_n, park, cseed, cfin)
  const bool five = e->alpha[0] == 0.0;
  const double* cseed = nullptr;                  // the first one or two reads of a pair from a table (DMX_CERTIFY_NO_SEEDS=1: the whole loop)
  if (five && !e->knob("DMX_CERTIFY_NO_SEEDS")) if (int rc = ensure_seeds(e, &cseed)) return rc;
  const double* cfin = nullptr;                   // final values of pairs of up to three tabled reads (DMX_CERTIFY_NO_FINALS=1 / DMX_CERTIFY_NO_SEEDS=1: none)
  if (cseed && !e->knob("DMX_CERTIFY_NO_FINALS")) if (int rc = ensure_finals(e, &cfin)) return rc;
  if (e->knob("DMX_CERTIFY_MINW3")) { if (gT) DMX_K3B(3, false, true); else DMX_K3B(3, false, false); }      // kernel experiments only
  else if (gT) { if (five) DMX_K3B(4, true, true); else DMX_K3B(4, false, true); }
  else { if (five) DMX_K3B(4, true, false); else DMX_K3B(4, false, false); }
#undef DMX_K3B
  HIP_TRY(hipGetLastError());
  return DMX_OK;
}
}  // namespace

extern "C" int dmx_engine_run_singlet(dmx_engine* e) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_run_singlet: null engine");
  if (!e->have_pileup || !e->d_g) return set_error(DMX_ERR_STATE, "dmx_engine_run_singlet: set genotypes and pileup first");
  HIP_TRY(hipSetDevice(e->device));
  if (e->pv.B == 0) { e->have_sing = true; return DMX_OK; }
  Event* rs = e->ring_s[e->n_ring_s % dmx_engine::kRing];
  e->k1_fn = nullptr;                              // dmx_engine_kernel_names: what THIS call launches, never an earlier call's choice
  HIP_TRY(hipEventRecord(e->ev[2], e->stream));
  HIP_TRY(hipEventRecord(rs[0], e->stream));
  if (int rc = launch_singlet(e)) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e->ev[3], e->stream));
  HIP_TRY(hipEventRecord(rs[1], e->stream));
  ++e->n_ring_s;
  e->timed[1] = true; e->have_sing = true; e->k1_placement = 0;
  return DMX_OK;
}

namespace { int run_doublet_impl(dmx_engine* e, bool with_singlet); }

extern "C" int dmx_engine_run_doublet(dmx_engine* e) { return run_doublet_impl(e, false); }

// K1 and K2 -> K3 -> K3b of the staged pileup in one call.  K3 reads nothing of K1's, so K1 runs BESIDE K2 on a stream of the lowest
// priority: K2's workgroups are dispatched first and K1 fills the slots K2 leaves free — above all during K2's last, partly filled
// round (cfg3 FAST: 10 000 one-barcode wavefronts on 3 072 slots).  Fork and join are events on the engine's stream, so that for the
// caller everything is ordered on that stream exactly as after run_singlet + run_doublet; the results are the same bits.
namespace {
// the doublet kernel launch_doublet picked is k_doublet_clsp (GT classes, grid {0, 0.5}, 33..64 samples): what launch_doublet itself recorded
bool k2_is_clsp(const dmx_engine* e) {
  return e->k2_fn == reinterpret_cast<const void*>(&k_doublet_clsp<3, false>) || e->k2_fn == reinterpret_cast<const void*>(&k_doublet_clsp<3, true>);
}
}  // namespace

extern "C" int dmx_engine_run(dmx_engine* e) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_run: null engine");
  // K1 beside K2 pays where K2 leaves slots free.  k_doublet_clsp does not (three wavefronts per SIMD, all of them issuing: measured on the
  // cfg4 shard, K1 beside it cost what it saved), so there K1 starts when K2 has finished and runs beside K3 + K3b (run_doublet_impl; cfg4 shard
  // 573 -> 566 ms per step).  DMX_FORCE_OVERLAP=1: beside K2 anyway; DMX_K1_FIRST=1: K1, then K2, K3, K3b, one after the other.
  const bool serial = e->knob("DMX_NO_OVERLAP") || e->knob("DMX_K1_FIRST");
  if (e->V < 2 || e->A < 2 || serial) {
    if (int rc = dmx_engine_run_singlet(e)) return rc;
    const int rc = (e->V < 2 || e->A < 2) ? DMX_OK : dmx_engine_run_doublet(e);
    e->k1_placement = 0;
    return rc;
  }
  return run_doublet_impl(e, true);
}

namespace {
int run_doublet_impl(dmx_engine* e, bool with_singlet) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_run_doublet: null engine");
  if (!e->have_pileup || !e->d_g) return set_error(DMX_ERR_STATE, "dmx_engine_run_doublet: set genotypes and pileup first");
  if (e->V < 2 || e->A < 2) return set_error(DMX_ERR_ARG, "dmx_engine_run_doublet: needs >= 2 samples and >= 2 alphas (got %d, %d)", e->V, e->A);
  HIP_TRY(hipSetDevice(e->device));
  const int32_t B = e->pv.B;
  const size_t nAB = (size_t)e->V * e->V * e->A;
  if (!e->d_grid || e->grid_cells < B) {
    e->d_grid.reset(); e->d_l00.reset(); e->d_sum.reset(); e->d_flag_base.reset(); e->d_sing.reset();
    const size_t cap = (size_t)e->out_cells;       // the singlet buffers' capacity (>= B)
    if (int rc = e->d_grid.alloc(std::max<size_t>(sizeof(double) * nAB * cap, 16))) return rc;
    if (int rc = e->d_l00.alloc(std::max<size_t>(sizeof(double) * (size_t)e->A * cap, 16))) return rc;
    if (int rc = e->d_sum.alloc(std::max<size_t>(sizeof(dmx_cell_summary) * cap, 16))) return rc;
    if (int rc = e->d_flag_base.alloc(cap + 2 * kFlagHead)) return rc;
    if (int rc = e->d_sing.alloc(std::max<size_t>(sizeof(double) * cap * e->V, 16))) return rc;
    e->grid_cells = (int32_t)cap;
  }
  e->k2_fn = e->k3b_fn = nullptr;                  // (dmx_engine_kernel_names reports this call's launches; a run without K3b leaves `certify` empty)
  if (with_singlet) e->k1_fn = nullptr;
  if (B == 0) { e->have_grid = true; if (with_singlet) e->have_sing = true; return DMX_OK; }
  Event* rd = e->ring_d[e->n_ring_d % dmx_engine::kRing];
  if (with_singlet) HIP_TRY(hipEventRecord(e->ev_fork, e->stream));       // (K1 must not start before what precedes this call on the stream)
  HIP_TRY(hipEventRecord(e->ev[4], e->stream));
  HIP_TRY(hipEventRecord(rd[0], e->stream));
  if (int rc = launch_doublet(e)) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e->ev[5], e->stream));
  HIP_TRY(hipEventRecord(rd[1], e->stream));
  if (with_singlet) {                            // K1, enqueued after K2, on the low-priority stream
    hipStream_t main_stream = e->stream;
    Event* rs = e->ring_s[e->n_ring_s % dmx_engine::kRing];
    // K1 beside K2 — or, where K2 leaves it no room (k_doublet_clsp: three issuing wavefronts per SIMD), beside K3 + K3b, which like K1
    // issue on about half of their cycles: K1 then starts when K2 has finished (DMX_FORCE_OVERLAP=1: beside K2 anyway)
    // The same holds for k_doublet_sym under ONE long K1 launch (round 5): its workgroups fill the CU's LDS three deep (46-53 KB each); a K1
    // workgroup (29 KB, alive for the whole launch) that takes the place of a retired one leaves no room for the next K2 workgroup, and the CU runs
    // two of K2's three until K1 ends — cfg3 FAST: K2 218 ms alone, 244 with a K1 beside it that takes 20 ms alone; step 260.5 -> 251.1 ms with K1
    // after K2.  A K1 walked in SNP blocks (sparse pileups over a matrix beyond the L2: a launch of short workgroups per block) does fit in
    // between: cfg5 FAST 49.0 ms beside K2, 53.2 after it.  STRICT's k_doublet_a2 keeps K1 beside it (cfg3 1 221.5 against 1 227.8, cfg5 144.2 / 150.2).
    const bool k1_blocked = e->pv.pair_snp != nullptr && e->blk_n > 1;
    const bool after_k2 = (k2_is_clsp(e) || (e->k2_sym && !k1_blocked) || e->knob("DMX_K1_AFTER_K2")) && !e->knob("DMX_FORCE_OVERLAP");
    e->k1_placement = after_k2 ? 2 : 1;
    HIP_TRY(hipStreamWaitEvent(e->k1_stream, after_k2 ? e->ev[5] : e->ev_fork, 0));
    e->stream = e->k1_stream;
    int rc = DMX_OK;
    hipError_t he = hipEventRecord(e->ev[2], e->stream);
    if (he == hipSuccess) he = hipEventRecord(rs[0], e->stream);
    if (he == hipSuccess) rc = launch_singlet(e);
    if (he == hipSuccess && rc == DMX_OK) he = hipGetLastError();
    if (he == hipSuccess && rc == DMX_OK) he = hipEventRecord(e->ev[3], e->stream);
    if (he == hipSuccess && rc == DMX_OK) he = hipEventRecord(rs[1], e->stream);
    if (he == hipSuccess && rc == DMX_OK) he = hipEventRecord(e->ev_k1_done, e->stream);
    e->stream = main_stream;
    if (rc != DMX_OK) return rc;
    HIP_TRY(he);
    ++e->n_ring_s;
    e->timed[1] = true; e->have_sing = true;
  }
  hipLaunchKernelGGL(k_reduce, dim3((unsigned)B), dim3(kThreads), 0, e->stream, e->d_grid, e->d_l00, e->pv.cell_pair_off,
                     e->d_alpha, e->V, e->A, e->prior, e->d_sum, e->d_sing);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(rd[2], e->stream));
  const bool certify = e->certify && e->A == 2 && e->alpha[1] == 0.5;
  if (certify) if (int rc = launch_certify(e)) return rc;
  HIP_TRY(hipEventRecord(e->ev[6], e->stream));
  HIP_TRY(hipEventRecord(rd[3], e->stream));
  e->ring_certified[e->n_ring_d % dmx_engine::kRing] = certify;
  ++e->n_ring_d;
  e->timed[2] = e->timed[3] = true; e->have_grid = true;
  if (with_singlet) HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_k1_done, 0));   // join: whatever follows on the stream sees K1's results
  return DMX_OK;
}
}  // namespace

extern "C" int dmx_engine_sync(dmx_engine* e) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_sync: null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return DMX_OK;
}

extern "C" int dmx_engine_get_singlet(dmx_engine* e, double* llks, double* llk0s) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_singlet: null engine");
  if (!e->have_sing) return set_error(DMX_ERR_STATE, "dmx_engine_get_singlet: run_singlet has not been called");
  HIP_TRY(hipSetDevice(e->device));
  const size_t B = (size_t)e->pv.B;
  if (llks && B) HIP_TRY(hipMemcpyAsync(llks, e->d_llks, sizeof(double) * B * e->V, hipMemcpyDeviceToHost, e->stream));
  if (llk0s && B) HIP_TRY(hipMemcpyAsync(llk0s, e->d_llk0s, sizeof(double) * B, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return DMX_OK;
}

extern "C" int dmx_engine_get_doublet(dmx_engine* e, double* llksAB, double* llks00, dmx_cell_summary* summary) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_doublet: null engine");
  if (!e->have_grid) return set_error(DMX_ERR_STATE, "dmx_engine_get_doublet: run_doublet has not been called");
  HIP_TRY(hipSetDevice(e->device));
  const size_t B = (size_t)e->pv.B, nAB = (size_t)e->V * e->V * e->A;
  if (llksAB && B) HIP_TRY(hipMemcpyAsync(llksAB, e->d_grid, sizeof(double) * B * nAB, hipMemcpyDeviceToHost, e->stream));
  if (llks00 && B) HIP_TRY(hipMemcpyAsync(llks00, e->d_l00, sizeof(double) * B * e->A, hipMemcpyDeviceToHost, e->stream));
  if (summary && B) HIP_TRY(hipMemcpyAsync(summary, e->d_sum, sizeof(dmx_cell_summary) * B, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return DMX_OK;
}

extern "C" int dmx_engine_get_sing(dmx_engine* e, double* sing) {
  if (!e || !sing) return set_error(DMX_ERR_ARG, "dmx_engine_get_sing: null argument");
  if (!e->have_grid) return set_error(DMX_ERR_STATE, "dmx_engine_get_sing: run_doublet has not been called");
  HIP_TRY(hipSetDevice(e->device));
  const size_t B = (size_t)e->pv.B;
  if (B) HIP_TRY(hipMemcpyAsync(sing, e->d_sing, sizeof(double) * B * e->V, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return DMX_OK;
}

extern "C" int dmx_engine_get_cell_grids(dmx_engine* e, const int32_t* cells, int32_t n, double* out) {
  if (!e || n < 0 || (n && (!cells || !out))) return set_error(DMX_ERR_ARG, "dmx_engine_get_cell_grids: bad arguments");
  if (!e->have_grid) return set_error(DMX_ERR_STATE, "dmx_engine_get_cell_grids: run_doublet has not been called");
  HIP_TRY(hipSetDevice(e->device));
  const size_t nAB = (size_t)e->V * e->V * e->A;
  for (int32_t i = 0; i < n; ++i)                  // every id before the first copy: an error must not leave copies into the caller's buffer in flight
    if (cells[i] < 0 || cells[i] >= e->pv.B) return set_error(DMX_ERR_ARG, "dmx_engine_get_cell_grids: cell %d out of range (0..%d)", cells[i], e->pv.B - 1);
  hipError_t he = hipSuccess;
  for (int32_t i = 0; i < n && he == hipSuccess; ++i)
    he = hipMemcpyAsync(out + (size_t)i * nAB, e->d_grid + (size_t)cells[i] * nAB, sizeof(double) * nAB, hipMemcpyDeviceToHost, e->stream);
  const hipError_t hs = hipStreamSynchronize(e->stream);                  // also after a failed copy: nothing stays in flight into `out`
  HIP_TRY(he);
  HIP_TRY(hs);
  return DMX_OK;
}

extern "C" int dmx_engine_device_view(dmx_engine* e, dmx_device_view* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_device_view: null argument");
  out->llks = e->d_llks; out->llk0s = e->d_llk0s; out->llksAB = e->d_grid; out->llks00 = e->d_l00; out->summary = e->d_sum;
  out->gp0s = e->d_gp0; out->sing = e->d_sing;
  return DMX_OK;
}

extern "C" int dmx_engine_last_kernel_times(dmx_engine* e, dmx_kernel_times* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_last_kernel_times: null argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  out->gp0_ms = out->singlet_ms = out->doublet_ms = out->reduce_ms = 0.f;
  if (e->timed[0]) HIP_TRY(hipEventElapsedTime(&out->gp0_ms, e->ev[0], e->ev[1]));
  if (e->timed[1]) HIP_TRY(hipEventElapsedTime(&out->singlet_ms, e->ev[2], e->ev[3]));
  if (e->timed[2]) HIP_TRY(hipEventElapsedTime(&out->doublet_ms, e->ev[4], e->ev[5]));
  if (e->timed[3]) HIP_TRY(hipEventElapsedTime(&out->reduce_ms, e->ev[5], e->ev[6]));
  return DMX_OK;
}

extern "C" int dmx_engine_mean_kernel_times(dmx_engine* e, int32_t reset, dmx_kernel_time_means* out) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_mean_kernel_times: null engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (out) {
    dmx_kernel_time_means m{};
    const int64_t ns = std::min<int64_t>(e->n_ring_s, dmx_engine::kRing), nd = std::min<int64_t>(e->n_ring_d, dmx_engine::kRing);
    for (int64_t i = 0; i < ns; ++i) {
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, e->ring_s[i][0], e->ring_s[i][1]));
      m.singlet_ms += ms / (double)ns;
    }
    for (int64_t i = 0; i < nd; ++i) {
      float a = 0.f, b = 0.f, c = 0.f;
      HIP_TRY(hipEventElapsedTime(&a, e->ring_d[i][0], e->ring_d[i][1]));
      HIP_TRY(hipEventElapsedTime(&b, e->ring_d[i][1], e->ring_d[i][2]));
      HIP_TRY(hipEventElapsedTime(&c, e->ring_d[i][2], e->ring_d[i][3]));
      m.doublet_ms += a / (double)nd; m.reduce_ms += b / (double)nd; m.certify_ms += c / (double)nd;
    }
    m.n_singlet = (int32_t)ns; m.n_doublet = (int32_t)nd;
    *out = m;
  }
  if (reset) e->n_ring_s = e->n_ring_d = 0;
  return DMX_OK;
}

extern "C" int dmx_engine_algorithmic_bytes(dmx_engine* e, dmx_kernel_bytes* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_algorithmic_bytes: null argument");
  if (!e->have_pileup) return set_error(DMX_ERR_STATE, "dmx_engine_algorithmic_bytes: no pileup staged");
  const double B = e->pv.B, V = e->V, A = e->A, S = e->S;
  // every input array once: pair counts + read bytes (+ SNP ids when sparse) + per-cell offsets and
  // launch order + the genotype matrix and gp0s once (they are L2/Infinity-Cache resident across cells)
  const double in = (double)e->P * e->nrd_width + (double)e->R + (e->pv.pair_snp ? 4.0 * (double)e->P : 0.0) +
                    (B + 1) * 16 + B * 4 + S * V * 12 + S * 24;
  out->singlet_bytes = in + B * (V + 1) * 8;
  out->doublet_bytes = in + B * (V * V * A + A) * 8;
  out->reduce_bytes = B * (V * V * A + A) * 8 + B * (double)sizeof(dmx_cell_summary);
  return DMX_OK;
}

namespace {
// "k_doublet_a2<256, 4, 4, true, false, 32>" — the demangled name rocprofv3 prints, without return type, namespace and parameter list
void kernel_name(const void* fn, char out[96]) {
  out[0] = 0;
  if (!fn) return;
  const char* mangled = hipKernelNameRefByPtr(fn, nullptr);
  if (!mangled) return;
  int st = 0;
  char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
  std::string n = (st == 0 && dem) ? dem : mangled;
  if (dem) std::free(dem);
  if (n.rfind("void ", 0) == 0) n.erase(0, 5);
  int depth = 0; size_t cut = n.size();                                  // the parameter list: the first '(' outside template brackets that is not "(anonymous namespace)"
  for (size_t i = 0; i < n.size(); ++i) {
    if (n[i] == '<') ++depth; else if (n[i] == '>') --depth;
    else if (n[i] == '(' && depth == 0 && n.compare(i, 21, "(anonymous namespace)") != 0) { cut = i; break; }
  }
  n.erase(cut);
  for (const char* pre : {"(anonymous namespace)::", "dmx::"}) for (size_t q; (q = n.find(pre)) != std::string::npos;) n.erase(q, std::strlen(pre));
  std::snprintf(out, 96, "%s", n.c_str());
}
}  // namespace

extern "C" int dmx_engine_kernel_names(dmx_engine* e, dmx_kernel_names* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_kernel_names: null argument");
  std::memset(out, 0, sizeof *out);
  kernel_name(e->k1_fn, out->singlet); kernel_name(e->k2_fn, out->doublet); kernel_name(e->k3b_fn, out->certify);
  out->k1_placement = e->k1_placement;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// What the feature calls' requests have in common ("Shared request helpers").  Every message names the calling entry point
// (fn).  The checks read the engine and never change it, so a refused call leaves every earlier result readable.
namespace {

int require_staged(dmx_engine* e, const char* fn) {
  if (!e->have_pileup) return set_error(DMX_ERR_STATE, "%s: no pileup staged (dmx_engine_set_pileup first)", fn);
  if (!e->d_g) return set_error(DMX_ERR_STATE, "%s: no genotype matrix (dmx_engine_set_genotypes first)", fn);
  if (e->pv.S != e->S)
    return set_error(DMX_ERR_STATE, "%s: the genotype matrix has %d SNPs, the staged pileup was checked against %d (stage it again)", fn, e->S, e->pv.S);
  return DMX_OK;
}

int require_sizes(dmx_engine* e, const char* fn, int32_t n_cells, int32_t n_snps) {
  if (n_cells != e->pv.B) return set_error(DMX_ERR_ARG, "%s: n_cells %d, the staged pileup has %d", fn, n_cells, e->pv.B);
  if (n_snps != e->S) return set_error(DMX_ERR_ARG, "%s: n_snps %d, the genotype matrix has %d", fn, n_snps, e->S);
  return DMX_OK;
}

// n ids from host or device memory into dst.  sync = false leaves a device copy pending on the stream, for a caller that waits for
// it together with copies of its own.
int fetch_ids(dmx_engine* e, const int32_t* src, int32_t memory, size_t n, std::vector<int32_t>& dst, bool sync = true) {
  dst.resize(n);
  if (n == 0) return DMX_OK;
  if (memory == DMX_MEM_DEVICE) {
    HIP_TRY(hipMemcpyAsync(dst.data(), src, sizeof(int32_t) * n, hipMemcpyDeviceToHost, e->stream));
    if (sync) HIP_TRY(hipStreamSynchronize(e->stream));
  } else {
    std::memcpy(dst.data(), src, sizeof(int32_t) * n);
  }
  return DMX_OK;
}

inline bool in_unit_interval(double x) { return x >= 0.0 && x <= 1.0; }   // (false for a NaN)
int not_in_unit_interval(const char* fn, const char* name, int32_t i, double x) {
  return set_error(DMX_ERR_ARG, "%s: %s[%d] = %g is not in [0, 1]", fn, name, i, x);
}
// p[n] (NULL = not given, nothing to check)
int check_unit_interval(const char* fn, const char* name, const double* p, int32_t n) {
  for (int32_t i = 0; p && i < n; ++i)
    if (!in_unit_interval(p[i])) return not_in_unit_interval(fn, name, i, p[i]);
  return DMX_OK;
}

// dst[n] on the device = src[n] of the host, or zeros where src is NULL (a soup that was not given)
int stage_soup(dmx_engine* e, const double* src, int32_t n, double* dst) {
  if (n <= 0) return DMX_OK;
  if (src) HIP_TRY(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, e->stream));
  else HIP_TRY(hipMemsetAsync(dst, 0, sizeof(double) * (size_t)n, e->stream));
  return DMX_OK;
}

// ids[n_slot][2], C slots per barcode: every slot is -1 (unused; counted out of *n_used) or two different samples in [0, V)
int check_pairs(const char* fn, const char* name, const std::vector<int32_t>& ids, size_t n_slot, int32_t C, int32_t V, int64_t* n_used) {
  *n_used = 0;
  for (size_t k = 0; k < n_slot; ++k) {
    const int32_t v1 = ids[2 * k], v2 = ids[2 * k + 1];
    if (v1 == -1) continue;
    if (v1 < 0 || v1 >= V || v2 < 0 || v2 >= V || v1 == v2)
      return set_error(DMX_ERR_ARG, "%s: %s[%zu][%zu] = (%d, %d) is not -1 or two different samples in [0, %d)", fn, name, k / (size_t)C, k % (size_t)C,
                       v1, v2, V);
    ++*n_used;
  }
  return DMX_OK;
}

// The hypotheses of dmx_engine_fit, dmx_engine_site_fit and dmx_engine_redraw: hyp[B][2] with alpha[B], rho[B] (NULL = 0) and the soup
// ambient[S] (NULL only with rho = NULL).  The caller runs check_args, check_ranges, the fetch of hyp, list and upload in this order
// with its own checks, buffers and device work between them; the plan lives until the call has synchronised (the uploads read it).
struct HypPlan {
  const char* fn;
  int32_t B, V, S;
  const int32_t* src; int32_t memory;              // the request's hyp and hyp_memory
  const double *alpha, *rho, *ambient;
  std::vector<int32_t> hyp, idx;                   // hyp on the host | the used barcodes, dmx::hyp_list_used's order
  std::vector<double> par;                         // alpha[B] | rho[B]
  int32_t n_sng = 0;

  int32_t n_used() const { return (int32_t)idx.size(); }
  int32_t n_dbl() const { return n_used() - n_sng; }
  int check_args() const {
    if (B > 0 && (!src || !alpha)) return set_error(DMX_ERR_ARG, "%s: missing hyp / alpha", fn);
    if (rho && !ambient && S > 0) return set_error(DMX_ERR_ARG, "%s: rho is given without ambient", fn);
    if (memory != DMX_MEM_HOST && memory != DMX_MEM_DEVICE) return set_error(DMX_ERR_ARG, "%s: hyp_memory %d", fn, memory);
    return DMX_OK;
  }
  int check_ranges() const {                       // (alpha and rho barcode by barcode: the first bad barcode is the one reported)
    for (int32_t b = 0; b < B; ++b) {
      const double al = alpha[b], rh = rho ? rho[b] : 0.0;
      if (!in_unit_interval(al)) return not_in_unit_interval(fn, "alpha", b, al);
      if (!in_unit_interval(rh)) return not_in_unit_interval(fn, "rho", b, rh);
    }
    return check_unit_interval(fn, "ambient", ambient, S);
  }
  int fetch(dmx_engine* e, bool sync = true) { return fetch_ids(e, src, memory, 2 * (size_t)B, hyp, sync); }
  int list() {
    const int32_t b = dmx::hyp_list_used(hyp.data(), B, V, idx, &n_sng);
    if (b >= 0)
      return set_error(DMX_ERR_ARG, "%s: hyp[%d] = (%d, %d) is not -1, a sample in [0, %d) or two different samples", fn, b, hyp[2 * (size_t)b],
                       hyp[2 * (size_t)b + 1], V);
    return DMX_OK;
  }
  int upload(dmx_engine* e, int32_t* d_hyp, double* d_par) {
    par.assign((size_t)B * 2, 0.0);
    for (int32_t b = 0; b < B; ++b) {
      par[(size_t)b] = alpha[b];
      if (rho) par[(size_t)B + b] = rho[b];
    }
    if (B == 0) return DMX_OK;
    HIP_TRY(hipMemcpyAsync(d_hyp, hyp.data(), sizeof(int32_t) * 2 * (size_t)B, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d_par, par.data(), sizeof(double) * 2 * (size_t)B, hipMemcpyHostToDevice, e->stream));
    return DMX_OK;
  }
};

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// Genotype refinement from called singlets.  The chunk plan is a counting sort of `assign` on the host (B ints);
// everything that touches the pileup runs on the device: k_snp_blocks (slab table, once per staged pileup), then per wave of chunks
// k_refine_partial + k_refine_fold, then k_refine_finish.
extern "C" int dmx_engine_refine_genotypes(dmx_engine* e, const dmx_refine_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_refine_genotypes: null argument");
  if (!e->have_pileup) return set_error(DMX_ERR_STATE, "dmx_engine_refine_genotypes: no pileup staged (dmx_engine_set_pileup first)");
  const int32_t B = e->pv.B, V = e->V, S = e->S;
  if (e->pv.S != S)
    return set_error(DMX_ERR_STATE, "dmx_engine_refine_genotypes: the genotype matrix has %d SNPs, the staged pileup was checked against %d (stage it again)", S, e->pv.S);
  if (int rc = require_sizes(e, "dmx_engine_refine_genotypes", rq->n_cells, rq->n_snps)) return rc;
  if ((B > 0 && !rq->assign) || (S > 0 && !rq->prior)) return set_error(DMX_ERR_ARG, "dmx_engine_refine_genotypes: missing assign / prior");
  if (rq->assign_memory != DMX_MEM_HOST && rq->assign_memory != DMX_MEM_DEVICE)
    return set_error(DMX_ERR_ARG, "dmx_engine_refine_genotypes: assign_memory %d", rq->assign_memory);
  if (!(rq->floor >= 0.0) || !std::isfinite(rq->floor)) return set_error(DMX_ERR_ARG, "dmx_engine_refine_genotypes: floor %g", rq->floor);
  HIP_TRY(hipSetDevice(e->device));
  for (Event& ev : e->rev) if (int rc = ev.create()) return rc;

  // ---- chunk plan: samp_chunk[V + 1] | chunk_beg[n_chunks + 1] | members[n_assigned] (cell ids by sample, ascending within a sample)
  std::vector<int32_t> a;
  if (int rc = fetch_ids(e, rq->assign, rq->assign_memory, (size_t)B, a)) return rc;
  std::vector<int64_t> cnt((size_t)V + 1, 0);
  for (int32_t b = 0; b < B; ++b) {
    if (a[(size_t)b] < -1 || a[(size_t)b] >= V) return set_error(DMX_ERR_ARG, "dmx_engine_refine_genotypes: assign[%d] = %d is not in [-1, %d)", b, a[(size_t)b], V);
    if (a[(size_t)b] >= 0) ++cnt[(size_t)a[(size_t)b] + 1];
  }
  for (int32_t v = 0; v < V; ++v) cnt[(size_t)v + 1] += cnt[(size_t)v];          // -> first member of each sample
  const int64_t n_asg = cnt[(size_t)V];
  std::vector<int32_t>& plan = e->h_rplan;
  plan.assign((size_t)V + 1, 0);
  for (int32_t v = 0; v < V; ++v) plan[(size_t)v + 1] = plan[(size_t)v] + (int32_t)((cnt[(size_t)v + 1] - cnt[(size_t)v] + kRefChunk - 1) / kRefChunk);
  const int32_t nch = plan[(size_t)V];
  for (int32_t v = 0; v < V; ++v)
    for (int32_t c = plan[(size_t)v]; c < plan[(size_t)v + 1]; ++c) plan.push_back((int32_t)(cnt[(size_t)v] + (int64_t)(c - plan[(size_t)v]) * kRefChunk));
  plan.push_back((int32_t)n_asg);
  const size_t o_beg = (size_t)V + 1, o_mem = o_beg + (size_t)nch + 1;
  plan.resize(o_mem + (size_t)n_asg);
  for (int32_t b = 0; b < B; ++b) if (a[(size_t)b] >= 0) plan[o_mem + (size_t)cnt[(size_t)a[(size_t)b]]++] = b;   // stable: ascending cell id

  const size_t rows = (size_t)S * V;
  if (int rc = e->d_rplan.ensure(sizeof(int32_t) * plan.size())) return rc;
  if (int rc = e->d_rprior.ensure(sizeof(float) * rows * 3)) return rc;
  if (int rc = e->d_rll.ensure(sizeof(double) * rows * 3)) return rc;
  if (int rc = e->d_rcnt.ensure(sizeof(int32_t) * rows * 3)) return rc;
  const int nxt = e->d_g == e->d_rgp[0] ? 1 : 0;                      // never the buffer the engine's genotype matrix is
  if (int rc = e->d_rgp[nxt].ensure(sizeof(float) * rows * 3)) return rc;
  HIP_TRY(hipMemcpyAsync(e->d_rplan, plan.data(), sizeof(int32_t) * plan.size(), hipMemcpyHostToDevice, e->stream));
  if (rows) HIP_TRY(hipMemcpyAsync(e->d_rprior, rq->prior, sizeof(float) * rows * 3, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemsetAsync(e->d_rll, 0, sizeof(double) * rows * 3, e->stream));
  HIP_TRY(hipMemsetAsync(e->d_rcnt, 0, sizeof(int32_t) * rows * 3, e->stream));

  // ---- slab table of the staged pileup (either layout): where every barcode stands at each slab boundary
  const int32_t nblk = (int32_t)(((int64_t)S + kRefSlab - 1) >> kRefSlabShift);
  const bool build_blk = !e->rblk_valid || e->rblk_S != S;
  HIP_TRY(hipEventRecord(e->rev[0], e->stream));
  if (build_blk && B > 0) {
    if (int rc = e->d_rblk.ensure(sizeof(int64_t) * 2 * (size_t)B * ((size_t)nblk + 1))) return rc;
    hipLaunchKernelGGL(k_snp_blocks, dim3((unsigned)((B + 3) / 4)), dim3(kThreads), 0, e->stream, e->pv, e->nrd_width, kRefSlabShift, nblk, e->d_rblk);
    HIP_TRY(hipGetLastError());
  }
  e->rblk_valid = true; e->rblk_S = S;
  HIP_TRY(hipEventRecord(e->rev[1], e->stream));

  // ---- partials, in waves of chunks that fit the budget (4 GiB, or a sixth of the free memory); the fold keeps the chunk order across waves
  const size_t per_chunk = sizeof(RefPartial) * (size_t)S;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const size_t budget = std::min<size_t>((size_t)4 << 30, free_b / 6);
  const int32_t cpw = (int32_t)std::max<size_t>(1, std::min<size_t>({per_chunk ? budget / per_chunk : (size_t)65535, (size_t)65535, (size_t)std::max(nch, 1)}));
  int32_t n_waves = 0;
  if (nch > 0 && S > 0) {
    if (int rc = e->d_rpart.ensure(per_chunk * (size_t)cpw)) return rc;
    const int32_t* d_samp = e->d_rplan;
    const int32_t* d_beg = e->d_rplan + o_beg;
    const int32_t* d_mem = e->d_rplan + o_mem;
    for (int32_t c0 = 0; c0 < nch; c0 += cpw, ++n_waves) {
      const int32_t nc = std::min(cpw, nch - c0);
      hipLaunchKernelGGL(k_refine_partial, dim3((unsigned)nblk, (unsigned)nc), dim3(64), 0, e->stream, e->pv, e->nrd_width, (const double*)e->d_lut,
                         (const int64_t*)e->d_rblk, nblk, d_mem, d_beg, c0, e->d_rpart.get());
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_refine_fold, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, e->stream, (const RefPartial*)e->d_rpart.get(), S, V, d_samp, c0,
                         c0 + nc, e->d_rll, e->d_rcnt);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipEventRecord(e->rev[2], e->stream));
  if (rows) {
    hipLaunchKernelGGL(k_refine_finish, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->d_rll, (const int32_t*)e->d_rcnt,
                       (const float*)e->d_rprior, (int64_t)rows, rq->floor, e->d_rgp[nxt]);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(e->rev[3], e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));        // the caller's prior may go away after return
  float ms[3] = {0.f, 0.f, 0.f};
  for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], e->rev[i], e->rev[i + 1]));
  dmx_refine_info& inf = e->ref_info;
  std::memset(&inf, 0, sizeof inf);
  inf.blocks_ms = build_blk ? ms[0] : 0.0; inf.partial_ms = ms[1]; inf.finish_ms = ms[2];
  inf.partial_bytes = nch > 0 ? (int64_t)(per_chunk * (size_t)cpw) : 0;
  inf.n_chunks = nch; inf.n_waves = n_waves; inf.chunk_cells = kRefChunk; inf.slab_snps = kRefSlab; inf.n_assigned = (int32_t)n_asg;
  e->rgp_cur = nxt; e->ref_S = S; e->have_refined = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_refined(dmx_engine* e, double* llk, int32_t* n_cell, int32_t* n_ref, int32_t* n_alt, float* gp) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_refined: null engine");
  if (!e->have_refined) return set_error(DMX_ERR_STATE, "dmx_engine_get_refined: no refinement on the staged pileup (dmx_engine_refine_genotypes first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t rows = (size_t)e->ref_S * e->V;
  if (!rows) return DMX_OK;
  if (llk) HIP_TRY(hipMemcpy(llk, e->d_rll, sizeof(double) * rows * 3, hipMemcpyDeviceToHost));
  if (n_cell) HIP_TRY(hipMemcpy(n_cell, e->d_rcnt, sizeof(int32_t) * rows, hipMemcpyDeviceToHost));
  if (n_ref) HIP_TRY(hipMemcpy(n_ref, e->d_rcnt + rows, sizeof(int32_t) * rows, hipMemcpyDeviceToHost));
  if (n_alt) HIP_TRY(hipMemcpy(n_alt, e->d_rcnt + 2 * rows, sizeof(int32_t) * rows, hipMemcpyDeviceToHost));
  if (gp) HIP_TRY(hipMemcpy(gp, e->d_rgp[e->rgp_cur], sizeof(float) * rows * 3, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_refined_device_ptr(dmx_engine* e, const float** out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_refined_device_ptr: null argument");
  if (!e->have_refined) return set_error(DMX_ERR_STATE, "dmx_engine_refined_device_ptr: no refinement on the staged pileup (dmx_engine_refine_genotypes first)");
  *out = e->d_rgp[e->rgp_cur];
  return DMX_OK;
}

extern "C" int dmx_engine_refine_info(dmx_engine* e, dmx_refine_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_refine_info: null argument");
  if (!e->have_refined) return set_error(DMX_ERR_STATE, "dmx_engine_refine_info: no refinement on the staged pileup (dmx_engine_refine_genotypes first)");
  *out = e->ref_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Genotype-free clustering: the stage cache, the M-step and the E-step of the EM that demuxlet_amd/cluster.py
// drives; K1 (dmx_engine_run_singlet) is the E-step's likelihood.
extern "C" int dmx_engine_cluster_stage(dmx_engine* e) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_stage: null engine");
  if (!e->have_pileup) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_stage: no pileup staged (dmx_engine_set_pileup first)");
  const int32_t B = e->pv.B, S = e->pv.S;
  HIP_TRY(hipSetDevice(e->device));
  int64_t po[2] = {0, 0};
  if (B > 0) {
    HIP_TRY(hipMemcpyAsync(&po[0], e->pv.cell_pair_off, sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(&po[1], e->pv.cell_pair_off + B, sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  const int64_t p_base = po[0], P = po[1] - po[0];
  const bool dense = e->pv.pair_snp == nullptr;
  if (!dense && P >= ((int64_t)1 << 31))
    return set_error(DMX_ERR_ARG, "dmx_engine_cluster_stage: %lld pairs; the sparse stage places pairs by 32-bit slots (below 2^31)", (long long)P);
  // the cache (32 bytes per pair) and, for a sparse layout, the placement's scratch: the slab table, the group counts M, the per-SNP
  // totals and the slot of every pair.  Groups of 64 barcodes, or more when M would pass 1 GiB.
  const int32_t nblk = (int32_t)(((int64_t)S + kClSlab - 1) >> kClSlabShift);
  int32_t gsz = 64;
  while ((double)((B + gsz - 1) / gsz) * S * sizeof(int32_t) > (double)(1u << 30)) gsz *= 2;
  const int32_t ng = (B + gsz - 1) / gsz;
  if (!dense && P > 0 && ng > 65535) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_stage: %d cells exceed this build's limit", B);
  const size_t cache_b = sizeof(int64_t) * ((size_t)S + 1) + (size_t)P * (sizeof(int32_t) + 3 * sizeof(double) + sizeof(uint32_t));
  const size_t scratch_b = (!dense && P > 0) ? 16 * (size_t)B * ((size_t)nblk + 1) + sizeof(int32_t) * ((size_t)ng * S + S + (size_t)P) : 0;
  e->d_coff.reset(); e->d_ccell.reset(); e->d_clgl.reset(); e->d_ccnt.reset();
  e->have_cstage = false;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if ((double)(cache_b + scratch_b) > 0.9 * (double)free_b)
    return set_error(DMX_ERR_NOMEM, "dmx_engine_cluster_stage: the cache of %lld pairs needs %.2f GB (+%.2f GB scratch), %.2f GB of device memory are free",
                     (long long)P, cache_b / 1e9, scratch_b / 1e9, free_b / 1e9);
  if (int rc = e->d_coff.ensure(sizeof(int64_t) * ((size_t)S + 1))) return rc;
  if (int rc = e->d_ccell.ensure(sizeof(int32_t) * (size_t)P)) return rc;
  if (int rc = e->d_clgl.ensure(3 * sizeof(double) * (size_t)P)) return rc;
  if (int rc = e->d_ccnt.ensure(sizeof(uint32_t) * (size_t)P)) return rc;
  std::vector<int64_t> off((size_t)S + 1, 0);
  DevBuf<int32_t> d_deep, d_M, d_tot, d_dst;     // the call's own scratch: freed on every return
  DevBuf<int64_t> d_sblk;
  if (int rc = d_deep.alloc(sizeof(int32_t))) return rc;
  HIP_TRY(hipMemsetAsync(d_deep, 0, sizeof(int32_t), e->stream));
  if (int rc = e->cev.record_start(e->stream)) return rc;
  if (dense) {
    const int64_t sp = B > 0 ? P / B : 0;                       // pairs per barcode (set_pileup checked that every barcode has them)
    for (int32_t t = 0; t <= S; ++t) off[(size_t)t] = std::min<int64_t>(t, sp) * B;
    HIP_TRY(hipMemcpyAsync(e->d_coff, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, e->stream));
  } else if (P == 0) {
    HIP_TRY(hipMemsetAsync(e->d_coff, 0, sizeof(int64_t) * ((size_t)S + 1), e->stream));
  } else {
    std::vector<int32_t> tot((size_t)S);
    if (int rc = d_sblk.alloc(16 * (size_t)B * ((size_t)nblk + 1))) return rc;
    if (int rc = d_M.alloc(sizeof(int32_t) * (size_t)ng * S)) return rc;
    if (int rc = d_tot.alloc(sizeof(int32_t) * (size_t)S)) return rc;
    if (int rc = d_dst.alloc(sizeof(int32_t) * (size_t)P)) return rc;
    hipLaunchKernelGGL(k_snp_blocks, dim3((unsigned)((B + 3) / 4)), dim3(kThreads), 0, e->stream, e->pv, e->nrd_width, kClSlabShift, nblk, d_sblk);
    hipLaunchKernelGGL(k_cluster_slots<false>, dim3((unsigned)nblk, (unsigned)ng), dim3(64), 0, e->stream, e->pv, (const int64_t*)d_sblk, nblk, gsz, p_base,
                       d_M, (const int64_t*)nullptr, (int32_t*)nullptr);
    hipLaunchKernelGGL(k_cluster_colscan, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, e->stream, d_M, ng, S, d_tot);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(tot.data(), d_tot, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int32_t t = 0; t < S; ++t) off[(size_t)t + 1] = off[(size_t)t] + tot[(size_t)t];
    if (off[(size_t)S] != P) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_stage: %lld pairs placed of %lld", (long long)off[(size_t)S], (long long)P);
    HIP_TRY(hipMemcpyAsync(e->d_coff, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_cluster_slots<true>, dim3((unsigned)nblk, (unsigned)ng), dim3(64), 0, e->stream, e->pv, (const int64_t*)d_sblk, nblk, gsz, p_base,
                       d_M, (const int64_t*)e->d_coff, d_dst);
    HIP_TRY(hipGetLastError());
  }
  if (B > 0) {
    hipLaunchKernelGGL(k_cluster_lgl, dim3((unsigned)((B + 3) / 4)), dim3(kThreads), 0, e->stream, e->pv, e->nrd_width, (const double*)e->d_lut, p_base,
                       (const int32_t*)d_dst, e->d_clgl, e->d_ccnt, e->d_ccell, d_deep);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->cev.record_stop(e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  int32_t deep = 0;
  HIP_TRY(hipMemcpy(&deep, d_deep, sizeof(int32_t), hipMemcpyDeviceToHost));
  if (deep) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_stage: a pair has more than 65 535 stored reads");
  float ms = 0.f;
  if (int rc = e->cev.elapsed_ms(&ms)) return rc;
  dmx_cluster_info& inf = e->cl_info;
  std::memset(&inf, 0, sizeof inf);
  inf.stage_ms = ms; inf.cache_bytes = (int64_t)cache_b; inf.n_pairs = P; inf.n_cells = B; inf.n_snps = S; inf.sorted = !dense && P > 0;
  inf.scratch_bytes = (int64_t)scratch_b;
  e->cl_P = P; e->cl_B = B; e->cl_S = S; e->have_cstage = true;
  e->have_cm = false; e->have_cw = false; e->have_ckw = false; e->have_khot = false; e->have_cdm = false;
  return DMX_OK;
}

namespace {

// Where an M-step takes its weights [B][C] from: the last E-step's (which must have had C columns), or the caller's, a host copy of
// which goes through d_cwh.  `last_estep` ends the message of the state error; `who` is the entry point.
int mstep_weights(dmx_engine* e, const char* who, const char* last_estep, int32_t memory, const double* weights, size_t nw, int32_t C, const double** w) {
  if (memory == DMX_CLUSTER_LAST_ESTEP) {
    if (!e->have_cw || e->cw_C != C) return set_error(DMX_ERR_STATE, "%s: no E-step weights of %s", who, last_estep);
    *w = e->d_cw;
  } else if (memory == DMX_MEM_HOST || memory == DMX_MEM_DEVICE) {
    if (nw > 0 && !weights) return set_error(DMX_ERR_ARG, "%s: missing weights", who);
    if (memory == DMX_MEM_HOST) {
      if (int rc = e->d_cwh.ensure(sizeof(double) * nw)) return rc;
      if (nw) HIP_TRY(hipMemcpyAsync(e->d_cwh, weights, sizeof(double) * nw, hipMemcpyHostToDevice, e->stream));
      *w = e->d_cwh;
    } else {
      *w = weights;
    }
  } else {
    return set_error(DMX_ERR_ARG, "%s: weights_memory %d", who, memory);
  }
  return DMX_OK;
}

// What the four E-steps share once their arguments are checked and their own inputs are on the device.  `launch(d_mask)` enqueues the
// variant's kernel, which fills d_cw (B x cw_cols), d_clse (B x R) and whatever else the variant keeps; the column sums of `w` (B x C:
// d_cw, or the known-column E-step's d_ckw), the log likelihoods of the R restarts and, with `dm`, the doublet masses then go
// through k_cluster_epart / k_cluster_efold and come back to the host.
struct EstepSums { double *col_sum, *ll, *dbl_mass; };
template <typename Launch>
int cluster_estep_run(dmx_engine* e, EventPair& ev, int32_t B, int32_t R, int32_t C, int32_t cw_cols, const DevBuf<double>& w, const DevBuf<double>* dm,
                      const uint8_t* mask, const EstepSums& sums, float* ms, Launch&& launch) {
  const int32_t nch = (B + kEChunk - 1) / kEChunk, ncol = C + (dm ? 2 : 1) * R;
  if (int rc = e->d_cw.ensure(sizeof(double) * (size_t)B * cw_cols)) return rc;
  if (int rc = e->d_clse.ensure(sizeof(double) * (size_t)B * R)) return rc;
  if (int rc = e->d_cpart.ensure(sizeof(double) * ((size_t)nch + 1) * ncol)) return rc;
  if (mask) if (int rc = e->d_cmask.ensure((size_t)B)) return rc;
  if (mask && B) HIP_TRY(hipMemcpyAsync(e->d_cmask, mask, (size_t)B, hipMemcpyHostToDevice, e->stream));
  double* d_out = e->d_cpart + (size_t)nch * ncol;   // (a view: the row behind the chunks' partials)
  if (int rc = ev.record_start(e->stream)) return rc;
  if (B > 0) {
    launch(mask ? (const uint8_t*)e->d_cmask : nullptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cluster_epart, dim3((unsigned)((ncol + 255) / 256), (unsigned)nch), dim3(256), 0, e->stream, (const double*)w,
                       (const double*)e->d_clse, dm ? (const double*)*dm : nullptr, B, C, R, e->d_cpart);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_cluster_efold, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->d_cpart, nch, ncol, d_out);
  HIP_TRY(hipGetLastError());
  if (int rc = ev.record_stop(e->stream)) return rc;
  std::vector<double> out((size_t)ncol);
  HIP_TRY(hipMemcpyAsync(out.data(), d_out, sizeof(double) * (size_t)ncol, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (sums.col_sum) std::memcpy(sums.col_sum, out.data(), sizeof(double) * (size_t)C);
  if (sums.ll) std::memcpy(sums.ll, out.data() + C, sizeof(double) * (size_t)R);
  if (dm && sums.dbl_mass) std::memcpy(sums.dbl_mass, out.data() + C + R, sizeof(double) * (size_t)R);
  e->have_cdm = dm != nullptr; e->cdm_B = B; e->cdm_R = R;   // (d_cdm is the last E-step's only after a doublet E-step)
  return ev.elapsed_ms(ms);
}

}  // namespace

extern "C" int dmx_engine_cluster_mstep(dmx_engine* e, const dmx_cluster_mstep_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_mstep: null argument");
  if (!e->have_cstage) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_mstep: no stage cache (dmx_engine_cluster_stage first)");
  const int32_t B = e->cl_B, S = e->cl_S, C = e->V;
  if (rq->n_cells != B || rq->n_snps != S) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_mstep: %d cells x %d SNPs, the stage cache has %d x %d", rq->n_cells, rq->n_snps, B, S);
  if (rq->n_cols != C) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_mstep: n_cols %d, the engine has %d columns", rq->n_cols, C);
  if (S > 0 && !rq->prior) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_mstep: missing prior");
  if (!(rq->floor >= 0.0) || !std::isfinite(rq->floor)) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_mstep: floor %g", rq->floor);
  HIP_TRY(hipSetDevice(e->device));
  const size_t nw = (size_t)B * C, rows = (size_t)S * C;
  const double* w = nullptr;
  if (int rc = mstep_weights(e, "dmx_engine_cluster_mstep", "this cache (dmx_engine_cluster_estep first)", rq->weights_memory, rq->weights, nw, C, &w)) return rc;
  if (int rc = e->d_cq.ensure(sizeof(float) * 3 * (size_t)S)) return rc;
  if (int rc = e->d_cll.ensure(sizeof(double) * 3 * rows)) return rc;
  if (int rc = e->d_cW.ensure(sizeof(double) * rows)) return rc;
  const int nxt = e->d_g == e->d_cgp[0] ? 1 : 0;                      // never the buffer the engine's genotype matrix is
  if (int rc = e->d_cgp[nxt].ensure(sizeof(float) * 3 * rows)) return rc;
  if (S) HIP_TRY(hipMemcpyAsync(e->d_cq, rq->prior, sizeof(float) * 3 * (size_t)S, hipMemcpyHostToDevice, e->stream));
  if (int rc = e->cev.record_start(e->stream)) return rc;
  if (rows) {
    hipLaunchKernelGGL(k_cluster_mstep, dim3((unsigned)((S + 3) / 4), (unsigned)((C + 63) / 64)), dim3(256), 0, e->stream, (const int64_t*)e->d_coff,
                       (const int32_t*)e->d_ccell, (const double*)e->d_clgl, w, S, C, (const float*)e->d_cq, rq->floor, e->d_cll, e->d_cW, e->d_cgp[nxt]);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->cev.record_stop(e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));        // the caller's prior / weights may go away after return
  float ms = 0.f;
  if (int rc = e->cev.elapsed_ms(&ms)) return rc;
  e->cl_info.mstep_ms = ms; e->cl_info.n_cols = C;
  e->cgp_cur = nxt; e->cm_S = S; e->cm_C = C; e->cgp_C = C; e->have_cm = true;
  return DMX_OK;
}

extern "C" int dmx_engine_cluster_estep(dmx_engine* e, const dmx_cluster_estep_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep: null argument");
  if (!e->have_cstage) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_estep: no stage cache (dmx_engine_cluster_stage first)");
  if (!e->have_sing) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_estep: no singlet likelihoods (dmx_engine_run_singlet first)");
  const int32_t B = e->pv.B, R = rq->n_restarts, K = rq->n_clusters, C = e->V;
  if (B != e->cl_B) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_estep: the staged pileup has %d cells, the stage cache %d", B, e->cl_B);
  if (R < 1 || K < 1 || (int64_t)R * K != C) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep: %d restarts x %d clusters, the engine has %d columns", R, K, C);
  if (!rq->log_pi) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep: missing log_pi");
  if (!(rq->temperature > 0.0) || !std::isfinite(rq->temperature)) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep: temperature %g", rq->temperature);
  const int32_t nch = (B + kEChunk - 1) / kEChunk;
  if (nch > 65535) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep: %d cells exceed this build's limit", B);
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = e->d_cpi.ensure(sizeof(double) * (size_t)C)) return rc;
  HIP_TRY(hipMemcpyAsync(e->d_cpi, rq->log_pi, sizeof(double) * (size_t)C, hipMemcpyHostToDevice, e->stream));
  float ms = 0.f;
  if (int rc = cluster_estep_run(e, e->cev, B, R, C, C, e->d_cw, nullptr, rq->mask, {rq->col_sum, rq->ll, nullptr}, &ms, [&](const uint8_t* d_mask) {
        hipLaunchKernelGGL(k_cluster_estep, dim3((unsigned)(((int64_t)B * R + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->d_llks, B, R, K,
                           (const double*)e->d_cpi, 1.0 / rq->temperature, d_mask, e->d_cw, e->d_clse);
      })) return rc;
  e->cl_info.estep_ms = ms;
  e->cw_C = C; e->have_cw = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_cluster(dmx_engine* e, double* ll, double* wsum, float* gp, double* weights) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_cluster: null engine");
  if ((ll || wsum || gp) && !e->have_cm) return set_error(DMX_ERR_STATE, "dmx_engine_get_cluster: no M-step on this stage cache (dmx_engine_cluster_mstep first)");
  if (weights && !e->have_cw) return set_error(DMX_ERR_STATE, "dmx_engine_get_cluster: no E-step on this stage cache (dmx_engine_cluster_estep first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t rows = (size_t)e->cm_S * e->cm_C, nw = (size_t)e->cl_B * e->cw_C;
  if (ll && rows) HIP_TRY(hipMemcpy(ll, e->d_cll, sizeof(double) * 3 * rows, hipMemcpyDeviceToHost));
  if (wsum && rows) HIP_TRY(hipMemcpy(wsum, e->d_cW, sizeof(double) * rows, hipMemcpyDeviceToHost));
  const size_t gp_rows = (size_t)e->cm_S * e->cgp_C;      // the windowed M-step's gp' has all V columns, its LL and W the free ones
  if (gp && gp_rows) HIP_TRY(hipMemcpy(gp, e->d_cgp[e->cgp_cur], sizeof(float) * 3 * gp_rows, hipMemcpyDeviceToHost));
  if (weights && nw) HIP_TRY(hipMemcpy(weights, e->d_cw, sizeof(double) * nw, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_get_cluster_stage(dmx_engine* e, int64_t* snp_off, int32_t* cell, double* lgl, uint32_t* ref_alt) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_cluster_stage: null engine");
  if (!e->have_cstage) return set_error(DMX_ERR_STATE, "dmx_engine_get_cluster_stage: no stage cache (dmx_engine_cluster_stage first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t P = (size_t)e->cl_P;
  if (snp_off) HIP_TRY(hipMemcpy(snp_off, e->d_coff, sizeof(int64_t) * ((size_t)e->cl_S + 1), hipMemcpyDeviceToHost));
  if (cell && P) HIP_TRY(hipMemcpy(cell, e->d_ccell, sizeof(int32_t) * P, hipMemcpyDeviceToHost));
  if (lgl && P) HIP_TRY(hipMemcpy(lgl, e->d_clgl, sizeof(double) * 3 * P, hipMemcpyDeviceToHost));
  if (ref_alt && P) HIP_TRY(hipMemcpy(ref_alt, e->d_ccnt, sizeof(uint32_t) * P, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_cluster_device_ptr(dmx_engine* e, const float** out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_device_ptr: null argument");
  if (!e->have_cm) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_device_ptr: no M-step on this stage cache (dmx_engine_cluster_mstep first)");
  *out = e->d_cgp[e->cgp_cur];
  return DMX_OK;
}

extern "C" int dmx_engine_cluster_info(dmx_engine* e, dmx_cluster_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_info: null argument");
  if (!e->have_cstage) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_info: no stage cache (dmx_engine_cluster_stage first)");
  *out = e->cl_info;
  return DMX_OK;
}

// Doublet-aware clustering: LLD of the pairs of clusters within each restart (k_cluster_dbl over B x
// ceil(R P / 64) wavefronts), then the E-step over K singlet and P doublet components whose sums go through k_cluster_epart /
// k_cluster_efold with R more columns.
extern "C" int dmx_engine_cluster_doublet(dmx_engine* e, int32_t n_restarts, int32_t n_clusters) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_doublet: null engine");
  if (int rc = require_staged(e, "dmx_engine_cluster_doublet")) return rc;
  const int32_t B = e->pv.B, R = n_restarts, K = n_clusters, V = e->V;
  if (K < 2 || K > 65535) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_doublet: %d clusters; the doublet components need 2 .. 65 535", K);
  if (R < 1 || (int64_t)R * K != V) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_doublet: %d restarts x %d clusters, the engine has %d columns", R, K, V);
  const int64_t P = (int64_t)K * (K - 1) / 2, ncols = (int64_t)R * P;
  if (ncols > INT32_MAX) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_doublet: %lld pair-columns exceed this build's limit", (long long)ncols);
  const int32_t n_cblk = (int32_t)((ncols + 63) / 64);
  const int64_t n_units = (int64_t)B * n_cblk;
  if ((n_units + kDblWaves - 1) / kDblWaves > INT32_MAX) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_doublet: %d cells x %lld pair-columns exceed this build's limit", B, (long long)ncols);
  HIP_TRY(hipSetDevice(e->device));
  const size_t lld_b = sizeof(double) * ((size_t)B * (size_t)ncols + (size_t)B), pairs_b = sizeof(uint32_t) * (size_t)P;   // LLD, then lsc[B]
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const size_t need = (lld_b > e->d_clld.cap() ? lld_b : 0) + (pairs_b > e->d_cpairs.cap() ? pairs_b : 0);
  if (need > 0 && (double)need > 0.9 * (double)free_b)
    return set_error(DMX_ERR_NOMEM, "dmx_engine_cluster_doublet: LLD of %d cells x %d restarts x %lld pairs needs %.2f GB (+%.2f MB pair table), %.2f GB of device memory are free",
                     B, R, (long long)P, lld_b / 1e9, pairs_b / 1e6, free_b / 1e9);
  e->have_cdbl = false;
  if (int rc = e->d_clld.ensure(lld_b)) return rc;
  if (int rc = e->d_cpairs.ensure(pairs_b)) return rc;
  std::vector<uint32_t> pr((size_t)P);
  for (int32_t k = 0, p = 0; k < K; ++k)
    for (int32_t l = k + 1; l < K; ++l) pr[(size_t)p++] = (uint32_t)k | ((uint32_t)l << 16);
  HIP_TRY(hipMemcpyAsync(e->d_cpairs, pr.data(), pairs_b, hipMemcpyHostToDevice, e->stream));
  if (int rc = e->dev_.record_start(e->stream)) return rc;
  if (n_units > 0) {
    hipLaunchKernelGGL(k_cluster_dbl, dim3((unsigned)((n_units + kDblWaves - 1) / kDblWaves)), dim3(64 * kDblWaves), 0, e->stream, e->pv, e->nrd_width,
                       (const double*)e->d_lut, (const float*)e->d_g, V, K, (int32_t)P, (const uint32_t*)e->d_cpairs, (int32_t)ncols, n_cblk, n_units,
                       e->d_clld, e->d_clld + (size_t)B * ncols);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->dev_.record_stop(e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  float ms = 0.f;
  if (int rc = e->dev_.elapsed_ms(&ms)) return rc;
  dmx_cluster_doublet_info& inf = e->cd_info;
  std::memset(&inf, 0, sizeof inf);
  inf.doublet_ms = ms; inf.lld_bytes = (int64_t)lld_b; inf.n_cells = B; inf.n_restarts = R; inf.n_clusters = K; inf.n_pairs = (int32_t)P;
  e->cd_B = B; e->cd_R = R; e->cd_K = K; e->have_cdbl = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_cluster_doublet(dmx_engine* e, double* lld, double* lsc) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_cluster_doublet: null engine");
  if (!e->have_cdbl) return set_error(DMX_ERR_STATE, "dmx_engine_get_cluster_doublet: no doublet likelihoods on the staged pileup (dmx_engine_cluster_doublet first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t n = (size_t)e->cd_B * e->cd_R * ((size_t)e->cd_K * (e->cd_K - 1) / 2);
  if (lld && n) HIP_TRY(hipMemcpy(lld, e->d_clld, sizeof(double) * n, hipMemcpyDeviceToHost));
  if (lsc && e->cd_B) HIP_TRY(hipMemcpy(lsc, e->d_clld + n, sizeof(double) * (size_t)e->cd_B, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_cluster_estep_doublet(dmx_engine* e, const dmx_cluster_estep_doublet_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_doublet: null argument");
  if (!e->have_cstage) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_estep_doublet: no stage cache (dmx_engine_cluster_stage first)");
  if (!e->have_sing) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_estep_doublet: no singlet likelihoods (dmx_engine_run_singlet first)");
  const int32_t B = e->pv.B, R = rq->n_restarts, K = rq->n_clusters, C = e->V;
  if (B != e->cl_B) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_estep_doublet: the staged pileup has %d cells, the stage cache %d", B, e->cl_B);
  if (K < 2 || R < 1 || (int64_t)R * K != C) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_doublet: %d restarts x %d clusters, the engine has %d columns", R, K, C);
  if (!e->have_cdbl || e->cd_B != B || e->cd_R != R || e->cd_K != K)
    return set_error(DMX_ERR_STATE, "dmx_engine_cluster_estep_doublet: no doublet likelihoods of %d restarts x %d clusters (dmx_engine_cluster_doublet first)", R, K);
  if (!rq->log_pi || !rq->log_delta) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_doublet: missing log_pi / log_delta");
  if (!(rq->temperature > 0.0) || !std::isfinite(rq->temperature)) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_doublet: temperature %g", rq->temperature);
  for (int32_t r = 0; r < R; ++r)
    if (!(rq->log_delta[r] < 0.0)) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_doublet: log_delta[%d] = %g; delta must be in [0, 1)", r, rq->log_delta[r]);
  const int32_t nch = (B + kEChunk - 1) / kEChunk;
  if (nch > 65535) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_doublet: %d cells exceed this build's limit", B);
  const int64_t P = (int64_t)K * (K - 1) / 2;
  // the log priors: singlet k  log(1 - delta) + log pi_k;  doublet (k, l)  log delta + log 2 + log pi_k + log pi_l - log(1 - sum pi^2)
  std::vector<double> lp((size_t)C + (size_t)R * P);
  double* lps = lp.data(); double* lpd = lp.data() + C;
  for (int32_t r = 0; r < R; ++r) {
    const double* pi = rq->log_pi + (size_t)r * K;
    const double ld = rq->log_delta[r], l1m = std::log1p(-std::exp(ld));
    double s2 = 0.0;
    for (int32_t k = 0; k < K; ++k) { lps[(size_t)r * K + k] = pi[k] + l1m; s2 += std::exp(2.0 * pi[k]); }
    const double lden = std::log1p(-s2);
    int64_t p = 0;
    for (int32_t k = 0; k < K; ++k)
      for (int32_t l = k + 1; l < K; ++l, ++p)
        lpd[(size_t)r * P + p] = (ld == -INFINITY || !(s2 < 1.0)) ? -INFINITY : ld + M_LN2 + pi[k] + pi[l] - lden;
  }
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = e->d_cdm.ensure(sizeof(double) * (size_t)B * R)) return rc;
  if (int rc = e->d_clp.ensure(sizeof(double) * lp.size())) return rc;
  HIP_TRY(hipMemcpyAsync(e->d_clp, lp.data(), sizeof(double) * lp.size(), hipMemcpyHostToDevice, e->stream));
  float ms = 0.f;
  if (int rc = cluster_estep_run(e, e->dev_, B, R, C, C, e->d_cw, &e->d_cdm, rq->mask, {rq->col_sum, rq->ll, rq->dbl_mass}, &ms, [&](const uint8_t* d_mask) {
        hipLaunchKernelGGL(k_cluster_estep_dbl, dim3((unsigned)(((int64_t)B * R + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->d_llks,
                           (const double*)e->d_clld, (const double*)(e->d_clld + (size_t)B * R * P), B, R, K, (int32_t)P, (const double*)e->d_clp, (const double*)(e->d_clp + C), 1.0 / rq->temperature,
                           d_mask, e->d_cw, e->d_clse, e->d_cdm);
      })) return rc;
  e->cd_info.estep_ms = ms;
  e->cw_C = C; e->have_cw = true;
  return DMX_OK;
}

extern "C" int dmx_engine_cluster_doublet_info(dmx_engine* e, dmx_cluster_doublet_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_doublet_info: null argument");
  if (!e->have_cdbl) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_doublet_info: no doublet likelihoods on the staged pileup (dmx_engine_cluster_doublet first)");
  *out = e->cd_info;
  return DMX_OK;
}

// Split-merge moves: the merge scores of the last M-step's columns (k_cluster_marg over S x C threads, then
// k_cluster_merge_part over ceil(S / kSmChunk) x R workgroups and k_cluster_merge_fold), and the grouped E-step, whose sums go through
// k_cluster_epart / k_cluster_efold as the plain E-step's do.
extern "C" int dmx_engine_cluster_merge_score(dmx_engine* e, int32_t n_restarts, int32_t n_clusters, const float* prior, double floor_,
                                              double* bf, int32_t* n_shared) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_merge_score: null engine");
  if (!e->have_cstage || !e->have_cm) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_merge_score: no M-step on this stage cache (dmx_engine_cluster_mstep first)");
  const int32_t R = n_restarts, K = n_clusters, S = e->cm_S, C = e->cm_C;
  if (K < 2 || K > kSmMaxK) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_merge_score: %d clusters; merge scores need 2 .. %d", K, kSmMaxK);
  if (R < 1 || (int64_t)R * K != C) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_merge_score: %d restarts x %d clusters, the last M-step has %d columns", R, K, C);
  if (R > 65535) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_merge_score: %d restarts exceed this build's limit", R);
  if (S > 0 && !prior) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_merge_score: missing prior");
  if (!(floor_ >= 0.0) || !std::isfinite(floor_)) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_merge_score: floor %g", floor_);
  const int32_t P = K * (K - 1) / 2, nch = (S + kSmChunk - 1) / kSmChunk;
  const size_t rows = (size_t)S * C, nout = (size_t)R * P, npart = (size_t)R * nch * P;
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = e->d_smA.ensure(sizeof(double) * rows)) return rc;
  if (int rc = e->d_smF.ensure(rows)) return rc;
  if (int rc = e->d_smq.ensure(sizeof(float) * 3 * (size_t)S)) return rc;
  if (int rc = e->d_smpart.ensure(sizeof(double) * npart)) return rc;
  if (int rc = e->d_smnpart.ensure(sizeof(int32_t) * npart)) return rc;
  if (int rc = e->d_smout.ensure(sizeof(double) * nout)) return rc;
  if (int rc = e->d_smnout.ensure(sizeof(int32_t) * nout)) return rc;
  if (S) HIP_TRY(hipMemcpyAsync(e->d_smq, prior, sizeof(float) * 3 * (size_t)S, hipMemcpyHostToDevice, e->stream));
  if (int rc = e->sev.record_start(e->stream)) return rc;
  if (rows) {
    hipLaunchKernelGGL(k_cluster_marg, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->d_cll, (const double*)e->d_cW,
                       (const float*)e->d_smq, floor_, S, C, e->d_smA, e->d_smF);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cluster_merge_part, dim3((unsigned)nch, (unsigned)R), dim3(256), 0, e->stream, (const double*)e->d_cll, (const double*)e->d_smA,
                       (const uint8_t*)e->d_smF, (const float*)e->d_smq, floor_, S, C, K, P, e->d_smpart, e->d_smnpart);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_cluster_merge_fold, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->d_smpart,
                     (const int32_t*)e->d_smnpart, nch, R, P, e->d_smout, e->d_smnout);
  HIP_TRY(hipGetLastError());
  if (int rc = e->sev.record_stop(e->stream)) return rc;
  if (bf) HIP_TRY(hipMemcpyAsync(bf, e->d_smout, sizeof(double) * nout, hipMemcpyDeviceToHost, e->stream));
  if (n_shared) HIP_TRY(hipMemcpyAsync(n_shared, e->d_smnout, sizeof(int32_t) * nout, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  float ms = 0.f;
  if (int rc = e->sev.elapsed_ms(&ms)) return rc;
  e->sm_info.merge_ms = ms; e->sm_info.n_restarts = R; e->sm_info.n_clusters = K; e->sm_info.n_pairs = P; e->sm_info.n_chunks = nch;
  return DMX_OK;
}

extern "C" int dmx_engine_cluster_estep_grouped(dmx_engine* e, const dmx_cluster_estep_grouped_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_grouped: null argument");
  if (!e->have_cstage) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_estep_grouped: no stage cache (dmx_engine_cluster_stage first)");
  if (!e->have_sing) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_estep_grouped: no singlet likelihoods (dmx_engine_run_singlet first)");
  const int32_t B = e->pv.B, R = rq->n_restarts, K = rq->n_clusters, C = e->V, Rs = rq->restarts_per_group;
  if (B != e->cl_B) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_estep_grouped: the staged pileup has %d cells, the stage cache %d", B, e->cl_B);
  if (R < 1 || K < 1 || (int64_t)R * K != C) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_grouped: %d restarts x %d clusters, the engine has %d columns", R, K, C);
  if (Rs < 1 || R % Rs != 0) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_grouped: %d restarts per group does not divide %d restarts", Rs, R);
  if (!rq->log_pi) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_grouped: missing log_pi");
  if (B > 0 && !rq->group) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_grouped: missing group");
  if (!(rq->temperature > 0.0) || !std::isfinite(rq->temperature)) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_grouped: temperature %g", rq->temperature);
  const int32_t G = R / Rs;
  for (int32_t b = 0; b < B; ++b)
    if (rq->group[b] < -1 || rq->group[b] >= G)
      return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_grouped: group[%d] = %d; groups are -1 .. %d", b, rq->group[b], G - 1);
  const int32_t nch = (B + kEChunk - 1) / kEChunk;
  if (nch > 65535) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_grouped: %d cells exceed this build's limit", B);
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = e->d_cpi.ensure(sizeof(double) * (size_t)C)) return rc;
  if (int rc = e->d_cgrp.ensure(sizeof(int32_t) * (size_t)B)) return rc;
  HIP_TRY(hipMemcpyAsync(e->d_cpi, rq->log_pi, sizeof(double) * (size_t)C, hipMemcpyHostToDevice, e->stream));
  if (B) HIP_TRY(hipMemcpyAsync(e->d_cgrp, rq->group, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, e->stream));
  float ms = 0.f;
  if (int rc = cluster_estep_run(e, e->sev, B, R, C, C, e->d_cw, nullptr, rq->mask, {rq->col_sum, rq->ll, nullptr}, &ms, [&](const uint8_t* d_mask) {
        hipLaunchKernelGGL(k_cluster_estep_grp, dim3((unsigned)(((int64_t)B * R + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->d_llks, B, R, K,
                           (const double*)e->d_cpi, 1.0 / rq->temperature, d_mask, (const int32_t*)e->d_cgrp, Rs, e->d_cw, e->d_clse);
      })) return rc;
  e->sm_info.grouped_estep_ms = ms;
  e->cw_C = C; e->have_cw = true;
  return DMX_OK;
}

extern "C" int dmx_engine_cluster_sm_info(dmx_engine* e, dmx_cluster_sm_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_sm_info: null argument");
  *out = e->sm_info;
  return DMX_OK;
}

// Choosing the number of clusters: the evidence of the last M-step's columns (k_cluster_marg, shared with the
// merge score and writing its d_smA / d_smF, then k_cluster_ev_part over ceil(S / kSmChunk) x ceil(C / 256) workgroups and
// k_cluster_ev_fold), the hard labels of the last E-step's weights with their ordered sums, and the in-place column merge.
extern "C" int dmx_engine_cluster_evidence(dmx_engine* e, int32_t n_restarts, int32_t n_clusters, const float* prior, double floor_, double* ev,
                                           int32_t* n_cov) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_evidence: null engine");
  if (!e->have_cstage || !e->have_cm) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_evidence: no M-step on this stage cache (dmx_engine_cluster_mstep first)");
  const int32_t R = n_restarts, K = n_clusters, S = e->cm_S, C = e->cm_C;
  if (K < 1 || K > kSmMaxK) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_evidence: %d clusters; the evidence needs 1 .. %d", K, kSmMaxK);
  if (R < 1 || (int64_t)R * K != C) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_evidence: %d restarts x %d clusters, the last M-step has %d columns", R, K, C);
  if (S > 0 && !prior) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_evidence: missing prior");
  if (!(floor_ >= 0.0) || !std::isfinite(floor_)) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_evidence: floor %g", floor_);
  const int32_t nch = (S + kSmChunk - 1) / kSmChunk;
  if (nch > 65535) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_evidence: %d SNPs exceed this build's limit", S);
  const size_t rows = (size_t)S * C, npart = ((size_t)nch + 1) * C;      // (the folded sums are the row behind the chunks' partials)
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = e->d_smA.ensure(sizeof(double) * rows)) return rc;
  if (int rc = e->d_smF.ensure(rows)) return rc;
  if (int rc = e->d_smq.ensure(sizeof(float) * 3 * (size_t)S)) return rc;
  if (int rc = e->d_kepart.ensure(sizeof(double) * npart)) return rc;
  if (int rc = e->d_kenpart.ensure(sizeof(int32_t) * npart)) return rc;
  double* d_ev = e->d_kepart + (size_t)nch * C;
  int32_t* d_nc = e->d_kenpart + (size_t)nch * C;
  if (S) HIP_TRY(hipMemcpyAsync(e->d_smq, prior, sizeof(float) * 3 * (size_t)S, hipMemcpyHostToDevice, e->stream));
  if (int rc = e->kkev.record_start(e->stream)) return rc;
  if (rows) {
    hipLaunchKernelGGL(k_cluster_marg, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->d_cll, (const double*)e->d_cW,
                       (const float*)e->d_smq, floor_, S, C, e->d_smA, e->d_smF);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cluster_ev_part, dim3((unsigned)((C + 255) / 256), (unsigned)nch), dim3(256), 0, e->stream, (const double*)e->d_smA,
                       (const uint8_t*)e->d_smF, S, C, e->d_kepart, e->d_kenpart);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_cluster_ev_fold, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->d_kepart,
                     (const int32_t*)e->d_kenpart, nch, C, d_ev, d_nc);
  HIP_TRY(hipGetLastError());
  if (int rc = e->kkev.record_stop(e->stream)) return rc;
  if (ev) HIP_TRY(hipMemcpyAsync(ev, d_ev, sizeof(double) * (size_t)C, hipMemcpyDeviceToHost, e->stream));
  if (n_cov) HIP_TRY(hipMemcpyAsync(n_cov, d_nc, sizeof(int32_t) * (size_t)C, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  float ms = 0.f;
  if (int rc = e->kkev.elapsed_ms(&ms)) return rc;
  e->k_info.evidence_ms = ms; e->k_info.n_restarts = R; e->k_info.n_clusters = K; e->k_info.n_chunks = nch;
  return DMX_OK;
}

extern "C" int dmx_engine_cluster_hard(dmx_engine* e, const dmx_cluster_hard_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_hard: null argument");
  if (!e->have_cstage || !e->have_cw) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_hard: no E-step weights on this stage cache (an E-step first)");
  const int32_t B = e->cl_B, R = rq->n_restarts, K = rq->n_clusters, C = e->cw_C;
  const bool dbl = rq->doublets != 0;
  if (R < 1 || K < 1 || (int64_t)R * K != C) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_hard: %d restarts x %d clusters, the last E-step's weights have %d columns", R, K, C);
  if (!rq->active) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_hard: missing active");
  for (int32_t r = 0; r < R; ++r) {
    int32_t n = 0;
    for (int32_t k = 0; k < K; ++k) n += rq->active[(size_t)r * K + k] != 0;
    if (n < (dbl ? 2 : 1))
      return set_error(DMX_ERR_ARG, "dmx_engine_cluster_hard: restart %d has %d active columns; %s", r, n, dbl ? "doublet labels need two" : "labels need one");
  }
  if (dbl && (!e->have_cdbl || e->cd_B != B || e->cd_R != R || e->cd_K != K))
    return set_error(DMX_ERR_STATE, "dmx_engine_cluster_hard: no doublet likelihoods of %d restarts x %d clusters (dmx_engine_cluster_doublet first)", R, K);
  if (dbl && (!e->have_cdm || e->cdm_B != B || e->cdm_R != R))
    return set_error(DMX_ERR_STATE, "dmx_engine_cluster_hard: the last E-step left no doublet mass (dmx_engine_cluster_estep_doublet first)");
  const int32_t nch = (B + kEChunk - 1) / kEChunk, ncol = C + R;
  if (nch > 65535) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_hard: %d cells exceed this build's limit", B);
  const int64_t P = (int64_t)K * (K - 1) / 2;
  HIP_TRY(hipSetDevice(e->device));
  e->have_khot = false;
  if (int rc = e->d_khot.ensure(sizeof(double) * (size_t)B * C)) return rc;
  if (int rc = e->d_klab.ensure(sizeof(int32_t) * (size_t)B * R)) return rc;
  if (int rc = e->d_kdsc.ensure(sizeof(double) * (size_t)B * R)) return rc;
  if (int rc = e->d_kact.ensure((size_t)C)) return rc;
  if (int rc = e->d_kipart.ensure(sizeof(int32_t) * ((size_t)nch + 1) * ncol)) return rc;
  if (int rc = e->d_kdpart.ensure(sizeof(double) * ((size_t)nch + 1) * R)) return rc;
  if (rq->mask) if (int rc = e->d_kmask.ensure((size_t)B)) return rc;
  std::vector<uint8_t> act((size_t)C);
  for (int32_t c = 0; c < C; ++c) act[(size_t)c] = rq->active[c] != 0;
  HIP_TRY(hipMemcpyAsync(e->d_kact, act.data(), (size_t)C, hipMemcpyHostToDevice, e->stream));
  if (rq->mask && B) HIP_TRY(hipMemcpyAsync(e->d_kmask, rq->mask, (size_t)B, hipMemcpyHostToDevice, e->stream));
  int32_t* d_iout = e->d_kipart + (size_t)nch * ncol;
  double* d_dout = e->d_kdpart + (size_t)nch * R;
  if (int rc = e->kkev.record_start(e->stream)) return rc;
  if (B > 0) {
    hipLaunchKernelGGL(k_cluster_hard, dim3((unsigned)(((int64_t)B * R + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->d_cw,
                       dbl ? (const double*)e->d_cdm : nullptr, dbl ? (const double*)e->d_clld : nullptr, (const uint8_t*)e->d_kact,
                       rq->mask ? (const uint8_t*)e->d_kmask : nullptr, B, R, K, (int32_t)P, e->d_klab, e->d_kdsc, e->d_khot);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cluster_hard_part, dim3((unsigned)((ncol + 255) / 256), (unsigned)nch), dim3(256), 0, e->stream, (const int32_t*)e->d_klab,
                       (const double*)e->d_kdsc, B, R, K, e->d_kipart, e->d_kdpart);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_cluster_hard_fold, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, e->stream, (const int32_t*)e->d_kipart,
                     (const double*)e->d_kdpart, nch, C, R, d_iout, d_dout);
  HIP_TRY(hipGetLastError());
  if (int rc = e->kkev.record_stop(e->stream)) return rc;
  std::vector<int32_t> iout((size_t)ncol);
  HIP_TRY(hipMemcpyAsync(iout.data(), d_iout, sizeof(int32_t) * (size_t)ncol, hipMemcpyDeviceToHost, e->stream));
  if (rq->dbl_score) HIP_TRY(hipMemcpyAsync(rq->dbl_score, d_dout, sizeof(double) * (size_t)R, hipMemcpyDeviceToHost, e->stream));
  if (rq->label && B) HIP_TRY(hipMemcpyAsync(rq->label, e->d_klab, sizeof(int32_t) * (size_t)B * R, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (rq->n_sing) std::memcpy(rq->n_sing, iout.data(), sizeof(int32_t) * (size_t)C);
  if (rq->n_dbl) std::memcpy(rq->n_dbl, iout.data() + C, sizeof(int32_t) * (size_t)R);
  float ms = 0.f;
  if (int rc = e->kkev.elapsed_ms(&ms)) return rc;
  e->k_info.hard_ms = ms; e->k_info.n_cells = B;
  e->khot_B = B; e->khot_C = C; e->khot_R = R; e->khot_dbl = dbl; e->have_khot = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_cluster_hard(dmx_engine* e, int32_t* label, double* score, double* hot, double* dbl_mass) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_cluster_hard: null engine");
  if (!e->have_khot) return set_error(DMX_ERR_STATE, "dmx_engine_get_cluster_hard: no hard labels on this stage cache (dmx_engine_cluster_hard first)");
  if (dbl_mass && !e->khot_dbl) return set_error(DMX_ERR_STATE, "dmx_engine_get_cluster_hard: the last hard labels read no doublet mass (doublets = 1 first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t B = (size_t)e->khot_B, C = (size_t)e->khot_C, R = (size_t)e->khot_R;
  if (label && B) HIP_TRY(hipMemcpy(label, e->d_klab, sizeof(int32_t) * B * R, hipMemcpyDeviceToHost));
  if (score && B) HIP_TRY(hipMemcpy(score, e->d_kdsc, sizeof(double) * B * R, hipMemcpyDeviceToHost));
  if (hot && B) HIP_TRY(hipMemcpy(hot, e->d_khot, sizeof(double) * B * C, hipMemcpyDeviceToHost));
  if (dbl_mass && B) HIP_TRY(hipMemcpy(dbl_mass, e->d_cdm, sizeof(double) * B * R, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_cluster_hard_device_ptr(dmx_engine* e, const double** out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_hard_device_ptr: null argument");
  if (!e->have_khot) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_hard_device_ptr: no hard labels on this stage cache (dmx_engine_cluster_hard first)");
  *out = e->d_khot;
  return DMX_OK;
}

extern "C" int dmx_engine_cluster_merge_columns(dmx_engine* e, int32_t n_restarts, int32_t n_clusters, const int32_t* from, const int32_t* into) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_merge_columns: null engine");
  if (!e->have_cstage || !e->have_cw) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_merge_columns: no E-step weights on this stage cache (an E-step first)");
  const int32_t B = e->cl_B, R = n_restarts, K = n_clusters, C = e->cw_C;
  if (R < 1 || K < 1 || (int64_t)R * K != C) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_merge_columns: %d restarts x %d clusters, the last E-step's weights have %d columns", R, K, C);
  if (!from || !into) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_merge_columns: missing from / into");
  std::vector<int32_t> fi((size_t)2 * R);
  for (int32_t r = 0; r < R; ++r) {
    if (from[r] < -1 || from[r] >= K) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_merge_columns: from[%d] = %d; columns are -1 .. %d", r, from[r], K - 1);
    if (from[r] >= 0 && (into[r] < 0 || into[r] >= K || into[r] == from[r]))
      return set_error(DMX_ERR_ARG, "dmx_engine_cluster_merge_columns: restart %d merges column %d into %d of %d", r, from[r], into[r], K);
    fi[(size_t)r] = from[r]; fi[(size_t)R + r] = from[r] >= 0 ? into[r] : 0;
  }
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = e->d_kfi.ensure(sizeof(int32_t) * fi.size())) return rc;
  HIP_TRY(hipMemcpyAsync(e->d_kfi, fi.data(), sizeof(int32_t) * fi.size(), hipMemcpyHostToDevice, e->stream));
  if (int rc = e->kkev.record_start(e->stream)) return rc;
  if (B > 0) {
    hipLaunchKernelGGL(k_cluster_merge_cols, dim3((unsigned)(((int64_t)B * R + 255) / 256)), dim3(256), 0, e->stream, e->d_cw.get(), (const int32_t*)e->d_kfi, B, R, K);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->kkev.record_stop(e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));        // (fi goes away after return)
  float ms = 0.f;
  if (int rc = e->kkev.elapsed_ms(&ms)) return rc;
  e->k_info.merge_columns_ms = ms;
  return DMX_OK;
}

extern "C" int dmx_engine_cluster_k_info(dmx_engine* e, dmx_cluster_k_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_k_info: null argument");
  *out = e->k_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Partly genotyped pools: Vk known columns shared by R restarts of M free ones.  The E-step is
// k_cluster_estep_known over B x R threads, whose sums over the R (Vk + M) components go through k_cluster_epart / k_cluster_efold; the
// M-step is k_cluster_mstep_win over the R M free columns, after a copy of the known rows into the gp' buffer it writes.
extern "C" int dmx_engine_cluster_set_known(dmx_engine* e, int32_t n_snps, int32_t n_known, const float* g, int32_t memory) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_set_known: null engine");
  if (n_snps < 0 || n_known < 0 || n_known >= e->V)
    return set_error(DMX_ERR_ARG, "dmx_engine_cluster_set_known: %d known columns of %d SNPs; the engine has %d columns and needs one free", n_known, n_snps, e->V);
  if (memory != DMX_MEM_HOST && memory != DMX_MEM_DEVICE) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_set_known: memory %d", memory);
  const size_t n = (size_t)n_snps * n_known * 3;
  if (n && !g) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_set_known: missing rows");
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = e->d_ckn.ensure(sizeof(float) * n)) return rc;
  if (n) HIP_TRY(hipMemcpyAsync(e->d_ckn, g, sizeof(float) * n, memory == DMX_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->ckn_S = n_snps; e->ckn_Vk = n_known; e->have_ckn = true;
  return DMX_OK;
}

extern "C" int dmx_engine_cluster_estep_known(dmx_engine* e, const dmx_cluster_estep_known_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_known: null argument");
  if (!e->have_cstage) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_estep_known: no stage cache (dmx_engine_cluster_stage first)");
  if (!e->have_sing) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_estep_known: no singlet likelihoods (dmx_engine_run_singlet first)");
  const int32_t B = e->pv.B, R = rq->n_restarts, Vk = rq->n_known, M = rq->n_free, V = e->V;
  if (B != e->cl_B) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_estep_known: the staged pileup has %d cells, the stage cache %d", B, e->cl_B);
  if (R < 1 || M < 1 || Vk < 0 || (int64_t)Vk + (int64_t)R * M != V)
    return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_known: %d known + %d restarts x %d free columns, the engine has %d columns", Vk, R, M, V);
  if (!rq->log_pi) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_known: missing log_pi");
  if (!(rq->temperature > 0.0) || !std::isfinite(rq->temperature)) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_known: temperature %g", rq->temperature);
  const int32_t nch = (B + kEChunk - 1) / kEChunk;
  if (nch > 65535) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_estep_known: %d cells exceed this build's limit", B);
  const int32_t K = Vk + M, CK = R * K, CF = R * M;
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = e->d_ckw.ensure(sizeof(double) * (size_t)B * CK)) return rc;
  if (int rc = e->d_cpi.ensure(sizeof(double) * (size_t)CK)) return rc;
  HIP_TRY(hipMemcpyAsync(e->d_cpi, rq->log_pi, sizeof(double) * (size_t)CK, hipMemcpyHostToDevice, e->stream));
  float ms = 0.f;
  if (int rc = cluster_estep_run(e, e->kev, B, R, CK, CF, e->d_ckw, nullptr, rq->mask, {rq->col_sum, rq->ll, nullptr}, &ms, [&](const uint8_t* d_mask) {
        hipLaunchKernelGGL(k_cluster_estep_known, dim3((unsigned)(((int64_t)B * R + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->d_llks, B, R,
                           Vk, M, (const double*)e->d_cpi, 1.0 / rq->temperature, d_mask, e->d_ckw, e->d_cw, e->d_clse);
      })) return rc;
  e->kn_info.estep_ms = ms; e->kn_info.n_cells = B; e->kn_info.n_known = Vk; e->kn_info.n_restarts = R; e->kn_info.n_free = M;
  e->cw_C = CF; e->have_cw = true;
  e->ckw_B = B; e->ckw_R = R; e->ckw_K = K; e->have_ckw = true;
  return DMX_OK;
}

extern "C" int dmx_engine_cluster_mstep_window(dmx_engine* e, const dmx_cluster_mstep_window_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_mstep_window: null argument");
  if (!e->have_cstage) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_mstep_window: no stage cache (dmx_engine_cluster_stage first)");
  if (!e->have_ckn) return set_error(DMX_ERR_STATE, "dmx_engine_cluster_mstep_window: no known rows (dmx_engine_cluster_set_known first)");
  const int32_t B = e->cl_B, S = e->cl_S, V = e->V, R = rq->n_restarts, M = rq->n_free, Vk = e->ckn_Vk;
  if (rq->n_cells != B || rq->n_snps != S) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_mstep_window: %d cells x %d SNPs, the stage cache has %d x %d", rq->n_cells, rq->n_snps, B, S);
  if (e->ckn_S != S) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_mstep_window: the known rows have %d SNPs, the stage cache %d", e->ckn_S, S);
  if (R < 1 || M < 1 || (int64_t)Vk + (int64_t)R * M != V)
    return set_error(DMX_ERR_ARG, "dmx_engine_cluster_mstep_window: %d known + %d restarts x %d free columns, the engine has %d columns", Vk, R, M, V);
  if (S > 0 && !rq->prior) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_mstep_window: missing prior");
  if (!(rq->floor >= 0.0) || !std::isfinite(rq->floor)) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_mstep_window: floor %g", rq->floor);
  HIP_TRY(hipSetDevice(e->device));
  const int32_t C = R * M;
  const size_t nw = (size_t)B * C, rows = (size_t)S * C;
  const double* w = nullptr;
  const std::string last = std::to_string(C) + " free columns (dmx_engine_cluster_estep_known first)";
  if (int rc = mstep_weights(e, "dmx_engine_cluster_mstep_window", last.c_str(), rq->weights_memory, rq->weights, nw, C, &w)) return rc;
  if (int rc = e->d_cq.ensure(sizeof(float) * 3 * (size_t)S)) return rc;
  if (int rc = e->d_cll.ensure(sizeof(double) * 3 * rows)) return rc;
  if (int rc = e->d_cW.ensure(sizeof(double) * rows)) return rc;
  const int nxt = e->d_g == e->d_cgp[0] ? 1 : 0;                      // never the buffer the engine's genotype matrix is
  if (int rc = e->d_cgp[nxt].ensure(sizeof(float) * 3 * (size_t)S * V)) return rc;
  if (S) HIP_TRY(hipMemcpyAsync(e->d_cq, rq->prior, sizeof(float) * 3 * (size_t)S, hipMemcpyHostToDevice, e->stream));
  if (int rc = e->kev.record_start(e->stream)) return rc;
  if (S && Vk)
    HIP_TRY(hipMemcpy2DAsync(e->d_cgp[nxt], sizeof(float) * 3 * (size_t)V, e->d_ckn, sizeof(float) * 3 * (size_t)Vk, sizeof(float) * 3 * (size_t)Vk,
                             (size_t)S, hipMemcpyDeviceToDevice, e->stream));
  if (rows) {
    hipLaunchKernelGGL(k_cluster_mstep_win, dim3((unsigned)((S + 3) / 4), (unsigned)((C + 63) / 64)), dim3(256), 0, e->stream, (const int64_t*)e->d_coff,
                       (const int32_t*)e->d_ccell, (const double*)e->d_clgl, w, S, C, (const float*)e->d_cq, rq->floor, e->d_cll, e->d_cW, e->d_cgp[nxt], Vk);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->kev.record_stop(e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));        // the caller's prior / weights may go away after return
  float ms = 0.f;
  if (int rc = e->kev.elapsed_ms(&ms)) return rc;
  e->kn_info.mstep_ms = ms; e->kn_info.n_known = Vk; e->kn_info.n_restarts = R; e->kn_info.n_free = M;
  e->cgp_cur = nxt; e->cm_S = S; e->cm_C = C; e->cgp_C = V; e->have_cm = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_cluster_known(dmx_engine* e, double* weights) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_cluster_known: null engine");
  if (weights && !e->have_ckw) return set_error(DMX_ERR_STATE, "dmx_engine_get_cluster_known: no known-column E-step (dmx_engine_cluster_estep_known first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t n = (size_t)e->ckw_B * e->ckw_R * e->ckw_K;
  if (weights && n) HIP_TRY(hipMemcpy(weights, e->d_ckw, sizeof(double) * n, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_cluster_known_info(dmx_engine* e, dmx_cluster_known_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_cluster_known_info: null argument");
  *out = e->kn_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Ambient contamination profile: the arguments are checked on the host (assign, a and the grid are small), then
// one launch of k_ambient over B x ceil(Q / 64) wavefronts.
extern "C" int dmx_engine_ambient(dmx_engine* e, const dmx_ambient_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_ambient: null argument");
  const char* fn = "dmx_engine_ambient";
  if (int rc = require_staged(e, fn)) return rc;
  const int32_t B = e->pv.B, V = e->V, S = e->S, Q = rq->n_grid;
  if (int rc = require_sizes(e, fn, rq->n_cells, rq->n_snps)) return rc;
  if (Q < 1 || Q > 256) return set_error(DMX_ERR_ARG, "dmx_engine_ambient: n_grid %d is not in [1, 256]", Q);
  if (!rq->grid || (B > 0 && !rq->assign) || (S > 0 && !rq->ambient)) return set_error(DMX_ERR_ARG, "dmx_engine_ambient: missing assign / ambient / grid");
  if (rq->assign_memory != DMX_MEM_HOST && rq->assign_memory != DMX_MEM_DEVICE)
    return set_error(DMX_ERR_ARG, "dmx_engine_ambient: assign_memory %d", rq->assign_memory);
  for (int32_t q = 0; q < Q; ++q) {
    const double r = rq->grid[q];
    if (!in_unit_interval(r)) return not_in_unit_interval(fn, "grid", q, r);
    if (q > 0 && !(r > rq->grid[q - 1])) return set_error(DMX_ERR_ARG, "dmx_engine_ambient: the grid is not strictly ascending at %d", q);
  }
  if (int rc = check_unit_interval(fn, "ambient", rq->ambient, S)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  std::vector<int32_t> a;
  if (int rc = fetch_ids(e, rq->assign, rq->assign_memory, (size_t)B, a)) return rc;
  int32_t n_asg = 0;
  for (int32_t b = 0; b < B; ++b) {
    if (a[(size_t)b] < -1 || a[(size_t)b] >= V) return set_error(DMX_ERR_ARG, "dmx_engine_ambient: assign[%d] = %d is not in [-1, %d)", b, a[(size_t)b], V);
    n_asg += a[(size_t)b] >= 0;
  }
  const size_t prof = sizeof(double) * (size_t)B * (size_t)Q;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (prof > e->d_all.cap() && prof + prof / 16 > free_b)
    return set_error(DMX_ERR_NOMEM, "dmx_engine_ambient: the %d x %d profile needs %zu bytes, %zu are free", B, Q, prof, free_b);
  if (int rc = e->d_all.ensure(prof)) return rc;
  if (int rc = e->d_acnt.ensure(sizeof(int32_t) * 2 * (size_t)B)) return rc;
  if (int rc = e->d_aasg.ensure(sizeof(int32_t) * (size_t)B)) return rc;
  if (int rc = e->d_aamb.ensure(sizeof(double) * (size_t)S)) return rc;
  if (int rc = e->d_agrid.ensure(sizeof(double) * (size_t)Q)) return rc;
  if (B > 0) HIP_TRY(hipMemcpyAsync(e->d_aasg, a.data(), sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, e->stream));
  if (int rc = stage_soup(e, rq->ambient, S, e->d_aamb)) return rc;
  HIP_TRY(hipMemcpyAsync(e->d_agrid, rq->grid, sizeof(double) * (size_t)Q, hipMemcpyHostToDevice, e->stream));
  const int32_t n_qblk = (Q + 63) / 64;
  const int64_t n_units = (int64_t)B * n_qblk;
  if (int rc = e->aev.record_start(e->stream)) return rc;
  if (n_units > 0) {
    hipLaunchKernelGGL(k_ambient, dim3((unsigned)((n_units + kAmbWaves - 1) / kAmbWaves)), dim3(64 * kAmbWaves), 0, e->stream, e->pv, e->nrd_width,
                       (const double*)e->d_lut, e->d_g, V, (const int32_t*)e->d_aasg, (const double*)e->d_aamb, (const double*)e->d_agrid, Q, n_qblk,
                       n_units, e->d_all, e->d_acnt, e->d_acnt + B);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->aev.record_stop(e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));        // the caller's inputs may go away after return
  float ms = 0.f;
  if (int rc = e->aev.elapsed_ms(&ms)) return rc;
  dmx_ambient_info& inf = e->amb_info;
  std::memset(&inf, 0, sizeof inf);
  inf.kernel_ms = ms; inf.profile_bytes = (int64_t)prof; inf.n_cells = B; inf.n_grid = Q; inf.n_assigned = n_asg;
  e->amb_B = B; e->amb_Q = Q; e->have_amb = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_ambient(dmx_engine* e, double* ll, int32_t* n_snp, int32_t* n_read) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_ambient: null engine");
  if (!e->have_amb) return set_error(DMX_ERR_STATE, "dmx_engine_get_ambient: no profile on the staged pileup (dmx_engine_ambient first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t B = (size_t)e->amb_B;
  if (!B) return DMX_OK;
  if (ll) HIP_TRY(hipMemcpy(ll, e->d_all, sizeof(double) * B * (size_t)e->amb_Q, hipMemcpyDeviceToHost));
  if (n_snp) HIP_TRY(hipMemcpy(n_snp, e->d_acnt, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
  if (n_read) HIP_TRY(hipMemcpy(n_read, e->d_acnt + B, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_ambient_info(dmx_engine* e, dmx_ambient_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_ambient_info: null argument");
  if (!e->have_amb) return set_error(DMX_ERR_STATE, "dmx_engine_ambient_info: no profile on the staged pileup (dmx_engine_ambient first)");
  *out = e->amb_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Ambient-aware doublet profile: the arguments are checked on the host (cand, a and the two grids are small), then
// one launch of k_ambient_dbl over B x A x ceil(Q / 64) wavefronts, instantiated for the smallest of 1 / 2 / 4 / 8 candidate slots that
// holds C.  Every buffer is the call's own: the last dmx_engine_ambient profile stays readable.
namespace {
template <int CC, int PT>
void launch_ambient_dbl(dmx_engine* e, int32_t C, int32_t A, int32_t Q, int32_t n_qblk, int64_t n_units) {
  hipLaunchKernelGGL((k_ambient_dbl<CC, PT>), dim3((unsigned)((n_units + kAmbDblWaves - 1) / kAmbDblWaves)), dim3(64 * kAmbDblWaves), 0, e->stream,
                     e->pv, e->nrd_width, (const double*)e->d_lut, e->d_g, e->V, (const int32_t*)e->d_dcand, C, (const double*)e->d_damb,
                     (const double*)(e->d_dgrid + Q), A, (const double*)e->d_dgrid, Q, n_qblk, n_units, e->d_dll, e->d_dcnt,
                     e->d_dcnt + (size_t)e->pv.B * C);
}
}  // namespace

extern "C" int dmx_engine_ambient_doublet(dmx_engine* e, const dmx_ambient_doublet_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_ambient_doublet: null argument");
  const char* fn = "dmx_engine_ambient_doublet";
  if (int rc = require_staged(e, fn)) return rc;
  const int32_t B = e->pv.B, V = e->V, S = e->S, C = rq->n_cand, A = rq->n_alpha, Q = rq->n_grid;
  if (int rc = require_sizes(e, fn, rq->n_cells, rq->n_snps)) return rc;
  if (C < 1 || C > kAmbDblMaxCand) return set_error(DMX_ERR_ARG, "dmx_engine_ambient_doublet: n_cand %d is not in [1, %d]", C, kAmbDblMaxCand);
  if (A < 1 || A > kAmbDblMaxAlpha) return set_error(DMX_ERR_ARG, "dmx_engine_ambient_doublet: n_alpha %d is not in [1, %d]", A, kAmbDblMaxAlpha);
  if (Q < 1 || Q > 256) return set_error(DMX_ERR_ARG, "dmx_engine_ambient_doublet: n_grid %d is not in [1, 256]", Q);
  if (!rq->grid || !rq->alpha || (B > 0 && !rq->cand) || (S > 0 && !rq->ambient))
    return set_error(DMX_ERR_ARG, "dmx_engine_ambient_doublet: missing cand / alpha / ambient / grid");
  if (rq->cand_memory != DMX_MEM_HOST && rq->cand_memory != DMX_MEM_DEVICE)
    return set_error(DMX_ERR_ARG, "dmx_engine_ambient_doublet: cand_memory %d", rq->cand_memory);
  for (int32_t n = 0; n < A; ++n) {
    const double x = rq->alpha[n];
    if (!in_unit_interval(x)) return not_in_unit_interval(fn, "alpha", n, x);
    if (n > 0 && !(x > rq->alpha[n - 1])) return set_error(DMX_ERR_ARG, "dmx_engine_ambient_doublet: alpha is not strictly ascending at %d", n);
  }
  for (int32_t q = 0; q < Q; ++q) {
    const double r = rq->grid[q];
    if (!in_unit_interval(r)) return not_in_unit_interval(fn, "grid", q, r);
    if (q > 0 && !(r > rq->grid[q - 1])) return set_error(DMX_ERR_ARG, "dmx_engine_ambient_doublet: the grid is not strictly ascending at %d", q);
  }
  if (int rc = check_unit_interval(fn, "ambient", rq->ambient, S)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  const size_t n_slot = (size_t)B * (size_t)C;
  std::vector<int32_t> cd;
  int64_t n_used = 0;
  if (int rc = fetch_ids(e, rq->cand, rq->cand_memory, 2 * n_slot, cd)) return rc;
  if (int rc = check_pairs(fn, "cand", cd, n_slot, C, V, &n_used)) return rc;
  const size_t prof = sizeof(double) * n_slot * (size_t)A * (size_t)Q;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (prof > e->d_dll.cap() && prof + prof / 16 > free_b)
    return set_error(DMX_ERR_NOMEM, "dmx_engine_ambient_doublet: the %d x %d x %d x %d profile needs %zu bytes, %zu are free", B, C, A, Q, prof, free_b);
  if (int rc = e->d_dll.ensure(prof)) return rc;
  if (int rc = e->d_dcnt.ensure(sizeof(int32_t) * 2 * n_slot)) return rc;
  if (int rc = e->d_dcand.ensure(sizeof(int32_t) * 2 * n_slot)) return rc;
  if (int rc = e->d_damb.ensure(sizeof(double) * (size_t)S)) return rc;
  if (int rc = e->d_dgrid.ensure(sizeof(double) * (size_t)(Q + A))) return rc;
  if (n_slot > 0) HIP_TRY(hipMemcpyAsync(e->d_dcand, cd.data(), sizeof(int32_t) * 2 * n_slot, hipMemcpyHostToDevice, e->stream));
  if (int rc = stage_soup(e, rq->ambient, S, e->d_damb)) return rc;
  HIP_TRY(hipMemcpyAsync(e->d_dgrid, rq->grid, sizeof(double) * (size_t)Q, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_dgrid + Q, rq->alpha, sizeof(double) * (size_t)A, hipMemcpyHostToDevice, e->stream));
  const int32_t n_qblk = (Q + 63) / 64;
  const int64_t n_units = (int64_t)B * A * n_qblk;
  if (int rc = e->dbev.record_start(e->stream)) return rc;
  if (n_units > 0) {
    if (C == 1) launch_ambient_dbl<1, 64>(e, C, A, Q, n_qblk, n_units);
    else if (C == 2) launch_ambient_dbl<2, 64>(e, C, A, Q, n_qblk, n_units);
    else if (C <= 4) launch_ambient_dbl<4, 32>(e, C, A, Q, n_qblk, n_units);
    else launch_ambient_dbl<8, 32>(e, C, A, Q, n_qblk, n_units);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->dbev.record_stop(e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));        // the caller's inputs may go away after return; cd is pageable host memory
  float ms = 0.f;
  if (int rc = e->dbev.elapsed_ms(&ms)) return rc;
  dmx_ambient_doublet_info& inf = e->adbl_info;
  std::memset(&inf, 0, sizeof inf);
  inf.kernel_ms = ms; inf.profile_bytes = (int64_t)prof; inf.n_used = n_used;
  inf.n_cells = B; inf.n_cand = C; inf.n_alpha = A; inf.n_grid = Q;
  e->adbl_B = B; e->adbl_C = C; e->adbl_A = A; e->adbl_Q = Q; e->have_adbl = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_ambient_doublet(dmx_engine* e, double* ll, int32_t* n_snp, int32_t* n_read) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_ambient_doublet: null engine");
  if (!e->have_adbl) return set_error(DMX_ERR_STATE, "dmx_engine_get_ambient_doublet: no profile on the staged pileup (dmx_engine_ambient_doublet first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t n_slot = (size_t)e->adbl_B * (size_t)e->adbl_C;
  if (!n_slot) return DMX_OK;
  if (ll) HIP_TRY(hipMemcpy(ll, e->d_dll, sizeof(double) * n_slot * (size_t)e->adbl_A * (size_t)e->adbl_Q, hipMemcpyDeviceToHost));
  if (n_snp) HIP_TRY(hipMemcpy(n_snp, e->d_dcnt, sizeof(int32_t) * n_slot, hipMemcpyDeviceToHost));
  if (n_read) HIP_TRY(hipMemcpy(n_read, e->d_dcnt + n_slot, sizeof(int32_t) * n_slot, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_ambient_doublet_info(dmx_engine* e, dmx_ambient_doublet_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_ambient_doublet_info: null argument");
  if (!e->have_adbl) return set_error(DMX_ERR_STATE, "dmx_engine_ambient_doublet_info: no profile on the staged pileup (dmx_engine_ambient_doublet first)");
  *out = e->adbl_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Triplet profile: the arguments are checked on the host (base and the shares are small), then one launch of
// k_triplet over B x C x T x ceil(V / (64 NACC)) wavefronts, NACC = 1 / 2 / 4 accumulators per lane by V alone.  Every buffer is the
// call's own.
namespace {
template <int NACC>
void launch_triplet(dmx_engine* e, int32_t C, int32_t T, int32_t n_vblk, int64_t n_units) {
  hipLaunchKernelGGL((k_triplet<NACC>), dim3((unsigned)((n_units + kTripWaves - 1) / kTripWaves)), dim3(64 * kTripWaves), 0, e->stream,
                     e->pv, e->nrd_width, (const double*)e->d_lut, e->d_g, e->V, (const int32_t*)e->d_tbase, C, (const double*)e->d_tshare, T,
                     n_vblk, n_units, e->d_tll, e->d_tcnt, e->d_tcnt + (size_t)e->pv.B * C * e->V);
}
}  // namespace

extern "C" int dmx_engine_triplet(dmx_engine* e, const dmx_triplet_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_triplet: null argument");
  const char* fn = "dmx_engine_triplet";
  if (int rc = require_staged(e, fn)) return rc;
  const int32_t B = e->pv.B, V = e->V, C = rq->n_base, T = rq->n_shares;
  if (int rc = require_sizes(e, fn, rq->n_cells, rq->n_snps)) return rc;
  if (C < 1 || C > kTripMaxSlot) return set_error(DMX_ERR_ARG, "dmx_engine_triplet: n_base %d is not in [1, %d]", C, kTripMaxSlot);
  if (T < 1 || T > kTripMaxShare) return set_error(DMX_ERR_ARG, "dmx_engine_triplet: n_shares %d is not in [1, %d]", T, kTripMaxShare);
  if (!rq->shares || (B > 0 && !rq->base)) return set_error(DMX_ERR_ARG, "dmx_engine_triplet: missing base / shares");
  if (rq->base_memory != DMX_MEM_HOST && rq->base_memory != DMX_MEM_DEVICE)
    return set_error(DMX_ERR_ARG, "dmx_engine_triplet: base_memory %d", rq->base_memory);
  for (int32_t t = 0; t < T; ++t) {
    const double* w = rq->shares + 3 * t;
    for (int k = 0; k < 3; ++k)
      if (!(w[k] >= 0.0 && w[k] <= 1.0)) return set_error(DMX_ERR_ARG, "dmx_engine_triplet: shares[%d][%d] = %g is not in [0, 1]", t, k, w[k]);
    if (!(std::fabs(w[0] + w[1] + w[2] - 1.0) <= 1e-12))
      return set_error(DMX_ERR_ARG, "dmx_engine_triplet: shares[%d] = (%g, %g, %g) do not sum to 1", t, w[0], w[1], w[2]);
    for (int32_t u = 0; u < t; ++u) {
      const double* x = rq->shares + 3 * u;
      if (x[0] == w[0] && x[1] == w[1] && x[2] == w[2]) return set_error(DMX_ERR_ARG, "dmx_engine_triplet: shares[%d] repeats shares[%d]", t, u);
    }
  }
  HIP_TRY(hipSetDevice(e->device));
  const size_t n_slot = (size_t)B * (size_t)C;
  std::vector<int32_t> bs;
  int64_t n_used = 0;
  if (int rc = fetch_ids(e, rq->base, rq->base_memory, 2 * n_slot, bs)) return rc;
  if (int rc = check_pairs(fn, "base", bs, n_slot, C, V, &n_used)) return rc;
  const size_t n_col = n_slot * (size_t)V;
  const size_t prof = sizeof(double) * n_col * (size_t)T, cnts = sizeof(int32_t) * 2 * n_col;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const size_t need = (prof > e->d_tll.cap() ? prof + prof / 16 : 0) + (cnts > e->d_tcnt.cap() ? cnts + cnts / 16 : 0);
  if (need > free_b)
    return set_error(DMX_ERR_NOMEM, "dmx_engine_triplet: the %d x %d x %d x %d profile needs %zu bytes, %zu are free", B, C, T, V, prof + cnts, free_b);
  if (int rc = e->d_tll.ensure(prof)) return rc;
  if (int rc = e->d_tcnt.ensure(cnts)) return rc;
  if (int rc = e->d_tbase.ensure(sizeof(int32_t) * 2 * n_slot)) return rc;
  if (int rc = e->d_tshare.ensure(sizeof(double) * 3 * (size_t)T)) return rc;
  if (n_slot > 0) HIP_TRY(hipMemcpyAsync(e->d_tbase, bs.data(), sizeof(int32_t) * 2 * n_slot, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_tshare, rq->shares, sizeof(double) * 3 * (size_t)T, hipMemcpyHostToDevice, e->stream));
  const int nacc = V <= 64 ? 1 : V <= 128 ? 2 : kTripMaxAcc;
  const int32_t n_vblk = (V + 64 * nacc - 1) / (64 * nacc);
  const int64_t n_units = (int64_t)n_slot * T * n_vblk;
  if (int rc = e->tev.record_start(e->stream)) return rc;
  if (n_units > 0) {
    if (nacc == 1) launch_triplet<1>(e, C, T, n_vblk, n_units);
    else if (nacc == 2) launch_triplet<2>(e, C, T, n_vblk, n_units);
    else launch_triplet<kTripMaxAcc>(e, C, T, n_vblk, n_units);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->tev.record_stop(e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));        // the caller's inputs may go away after return; bs is pageable host memory
  float ms = 0.f;
  if (int rc = e->tev.elapsed_ms(&ms)) return rc;
  dmx_triplet_info& inf = e->trip_info;
  std::memset(&inf, 0, sizeof inf);
  inf.kernel_ms = ms; inf.profile_bytes = (int64_t)prof; inf.n_used = n_used;
  inf.n_cells = B; inf.n_base = C; inf.n_shares = T; inf.n_samples = V;
  e->trip_B = B; e->trip_C = C; e->trip_T = T; e->trip_V = V; e->have_trip = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_triplet(dmx_engine* e, double* ll, int32_t* n_snp, int32_t* n_read) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_triplet: null engine");
  if (!e->have_trip) return set_error(DMX_ERR_STATE, "dmx_engine_get_triplet: no profile on the staged pileup (dmx_engine_triplet first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t n_col = (size_t)e->trip_B * (size_t)e->trip_C * (size_t)e->trip_V;
  if (!n_col) return DMX_OK;
  if (ll) HIP_TRY(hipMemcpy(ll, e->d_tll, sizeof(double) * n_col * (size_t)e->trip_T, hipMemcpyDeviceToHost));
  if (n_snp) HIP_TRY(hipMemcpy(n_snp, e->d_tcnt, sizeof(int32_t) * n_col, hipMemcpyDeviceToHost));
  if (n_read) HIP_TRY(hipMemcpy(n_read, e->d_tcnt + n_col, sizeof(int32_t) * n_col, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_triplet_info(dmx_engine* e, dmx_triplet_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_triplet_info: null argument");
  if (!e->have_trip) return set_error(DMX_ERR_STATE, "dmx_engine_triplet_info: no profile on the staged pileup (dmx_engine_triplet first)");
  *out = e->trip_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Anchored doublet search: the arguments are checked on the host, then k_anchor_col, k_anchor_select (unless the
// caller gave the anchors), k_anchor_pair and k_anchor_reduce on the engine's stream, each entry kernel over B x slabs wavefronts with
// NACC = 1 / 2 / 4 entries per lane by the entry count alone.  Every buffer is the call's own.
namespace {
template <int NACC>
void launch_anchor_col(dmx_engine* e, int A_pad, int TP, int32_t n_slab, int64_t n_units) {
  hipLaunchKernelGGL((k_anchor_col<NACC>), dim3((unsigned)((n_units + kAncWaves - 1) / kAncWaves)), dim3(64 * kAncWaves), 0, e->stream, e->pv,
                     e->nrd_width, e->d_g, (const double*)e->d_gp0, (const double*)e->d_lut, (const double*)e->d_alpha, e->V, e->A, A_pad, TP,
                     n_slab, n_units, (double*)e->d_ac0, (double*)e->d_al00);
}
template <int NACC>
void launch_anchor_pair(dmx_engine* e, int A_pad, int TP, int32_t T, int32_t n_slab, int64_t n_units) {
  hipLaunchKernelGGL((k_anchor_pair<NACC>), dim3((unsigned)((n_units + kAncWaves - 1) / kAncWaves)), dim3(64 * kAncWaves), 0, e->stream, e->pv,
                     e->nrd_width, e->d_g, (const double*)e->d_lut, (const double*)e->d_alpha, e->V, e->A, A_pad, TP, T,
                     (const int32_t*)e->d_anc, n_slab, n_units, (double*)e->d_apair);
}
inline int anchor_nacc(int64_t n_ent) { return n_ent <= 64 ? 1 : n_ent <= 128 ? 2 : 4; }
}  // namespace

extern "C" int dmx_engine_doublet_anchored(dmx_engine* e, const dmx_anchored_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_doublet_anchored: null argument");
  if (int rc = require_staged(e, "dmx_engine_doublet_anchored")) return rc;
  const int32_t B = e->pv.B, V = e->V, A = e->A, T = rq->n_anchor;
  if (V < 2 || A < 2) return set_error(DMX_ERR_ARG, "dmx_engine_doublet_anchored: %d samples x %d alphas; both must be at least 2", V, A);
  if (A > 64 || V > 0xFFE || (int64_t)V * V * A > 0x7FFFFFFFll)
    return set_error(DMX_ERR_ARG, "dmx_engine_doublet_anchored: %d samples x %d alphas exceed this build's limits (64 alphas, V*V*A < 2^31)", V, A);
  if (T < 1 || T > kAncMaxT || T > V) return set_error(DMX_ERR_ARG, "dmx_engine_doublet_anchored: n_anchor %d is not in [1, min(%d, V = %d)]", T, kAncMaxT, V);
  if (rq->n_cells != B) return set_error(DMX_ERR_ARG, "dmx_engine_doublet_anchored: n_cells %d, the staged pileup has %d", rq->n_cells, B);
  if (rq->anchors && rq->anchor_memory != DMX_MEM_HOST && rq->anchor_memory != DMX_MEM_DEVICE)
    return set_error(DMX_ERR_ARG, "dmx_engine_doublet_anchored: anchor_memory %d", rq->anchor_memory);
  if (!e->geno_rows_safe)
    return set_error(DMX_ERR_ARG, "dmx_engine_doublet_anchored: the genotype matrix has a row that is not finite, non-negative and above 1e-30 somewhere; "
                                  "run the full grid (dmx_engine_run_doublet), which has the fix-up pass for such a matrix: the anchored pass has none");
  HIP_TRY(hipSetDevice(e->device));
  const size_t n_anc = (size_t)B * (size_t)T;
  std::vector<int32_t> anc;
  int64_t n_used = (int64_t)n_anc;
  if (rq->anchors && n_anc > 0) {
    if (int rc = fetch_ids(e, rq->anchors, rq->anchor_memory, n_anc, anc)) return rc;
    n_used = 0;
    for (size_t b = 0; b < (size_t)B; ++b)
      for (int32_t t = 0; t < T; ++t) {
        const int32_t a = anc[b * T + t];
        if (a < -1 || a >= V) return set_error(DMX_ERR_ARG, "dmx_engine_doublet_anchored: anchors[%zu][%d] = %d is not -1 or a sample in [0, %d)", b, t, a, V);
        if (a < 0) continue;
        for (int32_t u = 0; u < t; ++u)
          if (anc[b * T + u] == a) return set_error(DMX_ERR_ARG, "dmx_engine_doublet_anchored: anchors[%zu][%d] repeats anchors[%zu][%d] = %d", b, t, b, u, a);
        ++n_used;
      }
  }
  const size_t c0_b = sizeof(double) * (size_t)B * V * A, pr_b = sizeof(double) * n_anc * V * 2 * (size_t)(A - 1),
               l00_b = sizeof(double) * (size_t)B * A, sum_b = sizeof(dmx_cell_summary) * (size_t)B, anc_b = sizeof(int32_t) * n_anc;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const size_t need = (c0_b > e->d_ac0.cap() ? c0_b + c0_b / 16 : 0) + (pr_b > e->d_apair.cap() ? pr_b + pr_b / 16 : 0) +
                      (l00_b > e->d_al00.cap() ? l00_b : 0) + (sum_b > e->d_asum.cap() ? sum_b : 0) + (anc_b > e->d_anc.cap() ? anc_b : 0);
  if (need > free_b)
    return set_error(DMX_ERR_NOMEM, "dmx_engine_doublet_anchored: the results of %d barcodes x %d samples x %d alphas x %d anchors need %zu bytes, %zu are free",
                     B, V, A, T, c0_b + pr_b + l00_b + sum_b + anc_b, free_b);
  if (int rc = e->d_ac0.ensure(c0_b)) return rc;
  if (int rc = e->d_apair.ensure(pr_b)) return rc;
  if (int rc = e->d_al00.ensure(l00_b)) return rc;
  if (int rc = e->d_asum.ensure(sum_b)) return rc;
  if (int rc = e->d_anc.ensure(anc_b)) return rc;
  e->have_anc = false;
  int A_pad = 1;
  while (A_pad < A) A_pad <<= 1;
  const int TP = std::min(kAncTP, 64 / A_pad);
  const int64_t ent_c = (int64_t)V * A, ent_p = (int64_t)T * 2 * (A - 1) * V;
  const int nacc_c = anchor_nacc(ent_c), nacc_p = anchor_nacc(ent_p);
  const int32_t slab_c = (int32_t)((ent_c + 64 * nacc_c - 1) / (64 * nacc_c)), slab_p = (int32_t)((ent_p + 64 * nacc_p - 1) / (64 * nacc_p));
  const int64_t units_c = (int64_t)B * slab_c, units_p = (int64_t)B * slab_p;
  if ((units_c + kAncWaves - 1) / kAncWaves > 0x7FFFFFFFll || (units_p + kAncWaves - 1) / kAncWaves > 0x7FFFFFFFll)
    return set_error(DMX_ERR_ARG, "dmx_engine_doublet_anchored: %d barcodes x %d samples need more wavefronts than one launch has", B, V);
  const unsigned cell_blocks = (unsigned)((B + kAncWaves - 1) / kAncWaves);
  if (int rc = e->anc_ev[0].record_start(e->stream)) return rc;
  if (B > 0) {
    if (nacc_c == 1) launch_anchor_col<1>(e, A_pad, TP, slab_c, units_c);
    else if (nacc_c == 2) launch_anchor_col<2>(e, A_pad, TP, slab_c, units_c);
    else launch_anchor_col<4>(e, A_pad, TP, slab_c, units_c);
    HIP_TRY(hipGetLastError());
    if (!anc.empty()) {
      HIP_TRY(hipMemcpyAsync(e->d_anc, anc.data(), anc_b, hipMemcpyHostToDevice, e->stream));
    } else {
      hipLaunchKernelGGL(k_anchor_select, dim3(cell_blocks), dim3(64 * kAncWaves), 0, e->stream, (const double*)e->d_ac0, B, V, A, T, (int32_t*)e->d_anc);
      HIP_TRY(hipGetLastError());
    }
  }
  if (int rc = e->anc_ev[0].record_stop(e->stream)) return rc;
  if (int rc = e->anc_ev[1].record_start(e->stream)) return rc;
  if (B > 0) {
    if (nacc_p == 1) launch_anchor_pair<1>(e, A_pad, TP, T, slab_p, units_p);
    else if (nacc_p == 2) launch_anchor_pair<2>(e, A_pad, TP, T, slab_p, units_p);
    else launch_anchor_pair<4>(e, A_pad, TP, T, slab_p, units_p);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->anc_ev[1].record_stop(e->stream)) return rc;
  if (int rc = e->anc_ev[2].record_start(e->stream)) return rc;
  if (B > 0) {
    hipLaunchKernelGGL(k_anchor_reduce, dim3(cell_blocks), dim3(64 * kAncWaves), 0, e->stream, (const double*)e->d_ac0, (const double*)e->d_apair,
                       (const double*)e->d_al00, (const int32_t*)e->d_anc, e->pv.cell_pair_off, (const double*)e->d_alpha, B, V, A, T, e->prior,
                       (dmx_cell_summary*)e->d_asum);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->anc_ev[2].record_stop(e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));        // the caller's anchors may go away after return; anc is pageable host memory
  if (anc.empty() && n_anc > 0) {                   // chosen on the device: a slot k_anchor_select left at -1 evaluated nothing
    anc.resize(n_anc);
    HIP_TRY(hipMemcpy(anc.data(), e->d_anc, anc_b, hipMemcpyDeviceToHost));
    n_used = 0;
    for (int32_t a : anc) n_used += a >= 0;
  }
  dmx_anchored_info& inf = e->anc_info;
  std::memset(&inf, 0, sizeof inf);
  float ms = 0.f;
  if (int rc = e->anc_ev[0].elapsed_ms(&ms)) return rc;
  inf.col_ms = ms;
  if (int rc = e->anc_ev[1].elapsed_ms(&ms)) return rc;
  inf.pair_ms = ms;
  if (int rc = e->anc_ev[2].elapsed_ms(&ms)) return rc;
  inf.reduce_ms = ms;
  inf.result_bytes = (int64_t)(c0_b + pr_b + l00_b + sum_b + anc_b);
  inf.n_entries = (int64_t)B * (ent_c + A) + n_used * (int64_t)(V - 1) * 2 * (A - 1);
  inf.n_cells = B; inf.n_samples = V; inf.n_alpha = A; inf.n_anchor = T;
  e->have_anc = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_anchored(dmx_engine* e, int32_t* anchors, double* c0, double* pairs, double* llks00, dmx_cell_summary* summary) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_anchored: null engine");
  if (!e->have_anc) return set_error(DMX_ERR_STATE, "dmx_engine_get_anchored: no anchored result (dmx_engine_doublet_anchored first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const dmx_anchored_info& inf = e->anc_info;
  const size_t B = (size_t)inf.n_cells, V = (size_t)inf.n_samples, A = (size_t)inf.n_alpha, T = (size_t)inf.n_anchor;
  if (!B) return DMX_OK;
  if (anchors) HIP_TRY(hipMemcpy(anchors, e->d_anc, sizeof(int32_t) * B * T, hipMemcpyDeviceToHost));
  if (c0) HIP_TRY(hipMemcpy(c0, e->d_ac0, sizeof(double) * B * V * A, hipMemcpyDeviceToHost));
  if (pairs) HIP_TRY(hipMemcpy(pairs, e->d_apair, sizeof(double) * B * T * V * 2 * (A - 1), hipMemcpyDeviceToHost));
  if (llks00) HIP_TRY(hipMemcpy(llks00, e->d_al00, sizeof(double) * B * A, hipMemcpyDeviceToHost));
  if (summary) HIP_TRY(hipMemcpy(summary, e->d_asum, sizeof(dmx_cell_summary) * B, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_anchored_info(dmx_engine* e, dmx_anchored_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_anchored_info: null argument");
  if (!e->have_anc) return set_error(DMX_ERR_STATE, "dmx_engine_anchored_info: no anchored result (dmx_engine_doublet_anchored first)");
  *out = e->anc_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Pileup composer (csrc/dmx_compose.hpp)
#include "dmx_compose.hpp"

extern "C" int dmx_engine_compose(dmx_engine* e, const dmx_compose_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_compose: null argument");
  if (rq->n_out < 1 || rq->n_out > dmx_cmp::kMaxOut)
    return set_error(DMX_ERR_ARG, "dmx_engine_compose: n_out %d is not in [1, %d] (compose a longer recipe in chunks by index_base)", rq->n_out, dmx_cmp::kMaxOut);
  if (!rq->parent || !rq->keep) return set_error(DMX_ERR_ARG, "dmx_engine_compose: missing parent / keep");
  if (!e->have_pileup) return set_error(DMX_ERR_STATE, "dmx_engine_compose: no pileup staged (dmx_engine_set_pileup first)");
  if (e->pv.cell_pair_off == (const int64_t*)e->d_cmpoff.get() && e->d_cmpoff)
    return set_error(DMX_ERR_STATE, "dmx_engine_compose: the staged pileup is this engine's own composed pileup (it would be overwritten)");
  const int32_t B = e->pv.B, N = rq->n_out;
  for (int32_t o = 0; o < N; ++o) {
    const int32_t p0 = rq->parent[2 * (size_t)o], p1 = rq->parent[2 * (size_t)o + 1];
    if (p0 < 0 || p0 >= B || p1 < -1 || p1 >= B)
      return set_error(DMX_ERR_ARG, "dmx_engine_compose: parent[%d] = (%d, %d) is not a cell in [0, %d) (slot 1: or -1)", o, p0, p1, B);
    for (int s = 0; s < 2; ++s)
      if (rq->keep[2 * (size_t)o + s] > dmx_cmp::kKeepAll)
        return set_error(DMX_ERR_ARG, "dmx_engine_compose: keep[%d][%d] = %llu is above 2^32", o, s, (unsigned long long)rq->keep[2 * (size_t)o + s]);
  }
  HIP_TRY(hipSetDevice(e->device));
  e->have_comp = false;
  // the parents' sizes, from the staged offsets: an upper bound of the result (checked against the free memory) and the algorithmic bytes
  std::vector<int64_t> h_po((size_t)B + 1), h_ro((size_t)B + 1);
  HIP_TRY(hipMemcpyAsync(h_po.data(), e->pv.cell_pair_off, sizeof(int64_t) * ((size_t)B + 1), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(h_ro.data(), e->pv.cell_read_off, sizeof(int64_t) * ((size_t)B + 1), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  int64_t src_pairs = 0, src_reads = 0;
  for (int32_t o = 0; o < N; ++o)
    for (int s = 0; s < 2; ++s) {
      const int32_t p = rq->parent[2 * (size_t)o + s];
      if (p >= 0) { src_pairs += h_po[(size_t)p + 1] - h_po[(size_t)p]; src_reads += h_ro[(size_t)p + 1] - h_ro[(size_t)p]; }
    }
  {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t have = e->d_cmsnp.cap() + e->d_cmnrd.cap() + e->d_cmreads.cap();
    const size_t worst = ((size_t)src_pairs * 8 + (size_t)src_reads + 64 * (size_t)N) * 17 / 16 + 4096;
    if (worst > have && worst - have > free_b)
      return set_error(DMX_ERR_NOMEM, "dmx_engine_compose: %d barcodes of up to %lld pairs and %lld reads may need %zu bytes, %zu are free",
                       N, (long long)src_pairs, (long long)src_reads, worst, free_b);
  }
  if (int rc = e->d_cmparent.ensure(sizeof(int32_t) * 2 * (size_t)N)) return rc;
  if (int rc = e->d_cmkeep.ensure(sizeof(uint64_t) * 2 * (size_t)N)) return rc;
  if (int rc = e->d_cmcnt.ensure(sizeof(int64_t) * (2 * (size_t)N + 3))) return rc;
  if (int rc = e->d_cmmax.ensure(sizeof(uint32_t) * (size_t)N)) return rc;
  if (int rc = e->d_cmpoff.ensure(sizeof(int64_t) * ((size_t)N + 1))) return rc;
  if (int rc = e->d_cmroff.ensure(sizeof(int64_t) * ((size_t)N + 1))) return rc;
  HIP_TRY(hipMemcpyAsync(e->d_cmparent, rq->parent, sizeof(int32_t) * 2 * (size_t)N, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_cmkeep, rq->keep, sizeof(uint64_t) * 2 * (size_t)N, hipMemcpyHostToDevice, e->stream));
  dmx_cmp::Ctx c{};
  c.pv = e->pv; c.nrd_width = e->nrd_width; c.n_out = N; c.index_base = rq->index_base; c.seed = rq->seed;
  c.parent = e->d_cmparent; c.keep = e->d_cmkeep;
  c.cnt_pairs = e->d_cmcnt; c.cnt_reads = e->d_cmcnt + N; c.cnt_max = e->d_cmmax;
  int64_t* d_totals = e->d_cmcnt + 2 * (size_t)N;
  const dim3 grid((unsigned)((N + dmx_cmp::kWaves - 1) / dmx_cmp::kWaves)), block(64 * dmx_cmp::kWaves);
  if (int rc = e->cmev[0].record_start(e->stream)) return rc;
  hipLaunchKernelGGL(dmx_cmp::k_compose<false>, grid, block, 0, e->stream, c);
  HIP_TRY(hipGetLastError());
  if (int rc = e->cmev[0].record_stop(e->stream)) return rc;
  if (int rc = e->cmev[1].record_start(e->stream)) return rc;
  hipLaunchKernelGGL(dmx_cmp::k_compose_scan, dim3(1), dim3(1024), 0, e->stream, (const int64_t*)c.cnt_pairs, (const int64_t*)c.cnt_reads,
                     (const uint32_t*)c.cnt_max, N, e->d_cmpoff.get(), e->d_cmroff.get(), d_totals);
  HIP_TRY(hipGetLastError());
  if (int rc = e->cmev[1].record_stop(e->stream)) return rc;
  int64_t totals[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(totals, d_totals, sizeof totals, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));        // the sizes decide the allocation and the width; rq's arrays may go away after return
  const int64_t P = totals[0], R = totals[1];
  if (P < 0 || R < 0 || P > src_pairs || R > src_reads)
    return set_error(DMX_ERR_HIP, "dmx_engine_compose: the count pass returned %lld pairs and %lld reads from %lld and %lld", (long long)P, (long long)R,
                     (long long)src_pairs, (long long)src_reads);
  const int need_w = totals[2] <= 0xFF ? 1 : totals[2] <= 0xFFFF ? 2 : 4;
  const int w = std::max(e->nrd_width, need_w);
  if (int rc = e->d_cmsnp.ensure(sizeof(int32_t) * (size_t)P + 16)) return rc;
  if (int rc = e->d_cmnrd.ensure((size_t)P * (size_t)w + 16)) return rc;
  if (int rc = e->d_cmreads.ensure((size_t)R + 64)) return rc;   // (slack: the lean K1 reads four bytes at a time)
  c.o_pair_off = e->d_cmpoff; c.o_read_off = e->d_cmroff;
  c.o_snp = e->d_cmsnp; c.o_nrd = e->d_cmnrd.get(); c.o_width = w; c.o_reads = e->d_cmreads;
  if (int rc = e->cmev[2].record_start(e->stream)) return rc;
  hipLaunchKernelGGL(dmx_cmp::k_compose<true>, grid, block, 0, e->stream, c);
  HIP_TRY(hipGetLastError());
  if (int rc = e->cmev[2].record_stop(e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  float ms[3] = {0.f, 0.f, 0.f};
  for (int i = 0; i < 3; ++i) if (int rc = e->cmev[i].elapsed_ms(&ms[i])) return rc;
  dmx_compose_info& inf = e->comp_info;
  std::memset(&inf, 0, sizeof inf);
  inf.n_pairs = P; inf.n_reads = R; inf.n_out = N; inf.nrd_width = w;
  inf.count_ms = ms[0]; inf.scan_ms = ms[1]; inf.fill_ms = ms[2];
  const int64_t src_pair_bytes = (e->pv.pair_snp ? 4 : 0) + e->nrd_width;
  inf.bytes_read = 2 * src_pairs * src_pair_bytes + R + 2 * (int64_t)N * 24 + (int64_t)N * 20 + 16 * ((int64_t)N + 1);
  inf.bytes_written = P * (4 + w) + R + (int64_t)N * 20 + 16 * ((int64_t)N + 1);
  e->have_comp = true;
  return DMX_OK;
}

extern "C" int dmx_engine_composed_pileup(dmx_engine* e, dmx_pileup* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_composed_pileup: null argument");
  if (!e->have_comp) return set_error(DMX_ERR_STATE, "dmx_engine_composed_pileup: nothing composed on the staged pileup (dmx_engine_compose first)");
  std::memset(out, 0, sizeof *out);
  out->n_cells = e->comp_info.n_out; out->n_snps = e->pv.S;
  out->n_pairs = e->comp_info.n_pairs; out->n_reads = e->comp_info.n_reads;
  out->cell_pair_off = e->d_cmpoff; out->cell_read_off = e->d_cmroff;
  out->pair_snp = e->d_cmsnp; out->pair_nrd = e->d_cmnrd.get(); out->nrd_width = e->comp_info.nrd_width;
  out->memory = DMX_MEM_DEVICE; out->reads = e->d_cmreads;
  return DMX_OK;
}

extern "C" int dmx_engine_get_composed(dmx_engine* e, int64_t* cell_pair_off, int64_t* cell_read_off, int32_t* pair_snp, void* pair_nrd, uint8_t* reads) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_composed: null engine");
  if (!e->have_comp) return set_error(DMX_ERR_STATE, "dmx_engine_get_composed: nothing composed on the staged pileup (dmx_engine_compose first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t N = (size_t)e->comp_info.n_out, P = (size_t)e->comp_info.n_pairs, R = (size_t)e->comp_info.n_reads, w = (size_t)e->comp_info.nrd_width;
  if (cell_pair_off) HIP_TRY(hipMemcpy(cell_pair_off, e->d_cmpoff, sizeof(int64_t) * (N + 1), hipMemcpyDeviceToHost));
  if (cell_read_off) HIP_TRY(hipMemcpy(cell_read_off, e->d_cmroff, sizeof(int64_t) * (N + 1), hipMemcpyDeviceToHost));
  if (pair_snp && P) HIP_TRY(hipMemcpy(pair_snp, e->d_cmsnp, sizeof(int32_t) * P, hipMemcpyDeviceToHost));
  if (pair_nrd && P) HIP_TRY(hipMemcpy(pair_nrd, e->d_cmnrd, P * w, hipMemcpyDeviceToHost));
  if (reads && R) HIP_TRY(hipMemcpy(reads, e->d_cmreads, R, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_compose_info(dmx_engine* e, dmx_compose_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_compose_info: null argument");
  if (!e->have_comp) return set_error(DMX_ERR_STATE, "dmx_engine_compose_info: nothing composed on the staged pileup (dmx_engine_compose first)");
  *out = e->comp_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Donor shares of a read pool.  census_prepare checks the arguments, sorts the barcodes by group (ascending cell
// id within a group), cuts each group into chunks of kCenChunk, uploads the plan and builds the dosage table; census_pass is one
// k_census_step + k_census_fold at the given shares for the active groups, with G (V + 3) doubles copied back.
namespace {

struct CensusPlan {
  int32_t G = 0, V = 0, n_chunks = 0;
  std::vector<int32_t> chunk_off;                // [G + 1]
};

int census_prepare(dmx_engine* e, const char* fn, int32_t n_cells, int32_t group_memory, const int32_t* group, int32_t G, int32_t n_samples,
                   CensusPlan* plan) {
  if (int rc = require_staged(e, fn)) return rc;
  const int32_t B = e->pv.B, V = e->V, S = e->S;
  if (n_cells != B) return set_error(DMX_ERR_ARG, "%s: n_cells %d, the staged pileup has %d", fn, n_cells, B);
  if (n_samples != V) return set_error(DMX_ERR_ARG, "%s: n_samples %d, the engine has %d", fn, n_samples, V);
  if (V > kCenMaxV) return set_error(DMX_ERR_ARG, "%s: %d samples, at most %d", fn, V, kCenMaxV);
  if (G < 1 || G > kCenMaxG) return set_error(DMX_ERR_ARG, "%s: n_groups %d is not in [1, %d]", fn, G, kCenMaxG);
  if (B > 0 && !group) return set_error(DMX_ERR_ARG, "%s: missing group", fn);
  if (group_memory != DMX_MEM_HOST && group_memory != DMX_MEM_DEVICE) return set_error(DMX_ERR_ARG, "%s: group_memory %d", fn, group_memory);
  HIP_TRY(hipSetDevice(e->device));
  std::vector<int32_t> grp;
  if (int rc = fetch_ids(e, group, group_memory, (size_t)B, grp)) return rc;
  std::vector<int32_t> n_in((size_t)G + 1, 0);
  for (int32_t b = 0; b < B; ++b) {
    if (grp[(size_t)b] < -1 || grp[(size_t)b] >= G) return set_error(DMX_ERR_ARG, "%s: group[%d] = %d is not in [-1, %d)", fn, b, grp[(size_t)b], G);
    if (grp[(size_t)b] >= 0) n_in[(size_t)grp[(size_t)b] + 1] += 1;
  }
  for (int32_t g = 0; g < G; ++g) n_in[(size_t)g + 1] += n_in[(size_t)g];          // first index of each group in the sorted list
  std::vector<int32_t> order((size_t)n_in[(size_t)G]), fill(n_in.begin(), n_in.end() - 1);
  for (int32_t b = 0; b < B; ++b) if (grp[(size_t)b] >= 0) order[(size_t)fill[(size_t)grp[(size_t)b]]++] = b;
  std::vector<CenChunk> chunks;
  plan->chunk_off.assign((size_t)G + 1, 0);
  for (int32_t g = 0; g < G; ++g) {
    for (int32_t i = n_in[(size_t)g]; i < n_in[(size_t)g + 1]; i += kCenChunk)
      chunks.push_back(CenChunk{g, i, std::min(kCenChunk, n_in[(size_t)g + 1] - i), 0});
    plan->chunk_off[(size_t)g + 1] = (int32_t)chunks.size();
  }
  plan->G = G; plan->V = V; plan->n_chunks = (int32_t)chunks.size();
  const size_t dos = sizeof(double) * (size_t)S * (size_t)V, par = sizeof(double) * chunks.size() * ((size_t)V + 1);
  size_t free_b = 0, total_b = 0, need = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (dos > e->d_cnd.cap()) need += dos + dos / 16;
  if (par > e->d_cnpart.cap()) need += par + par / 16;
  if (need > free_b)
    return set_error(DMX_ERR_NOMEM, "%s: the %d x %d dosage table and %zu chunk partials need %zu bytes, %zu are free", fn, S, V, chunks.size(), need, free_b);
  if (int rc = e->d_cnd.ensure(dos)) return rc;
  if (int rc = e->d_cnvalid.ensure((size_t)S)) return rc;
  if (int rc = e->d_cnpart.ensure(par)) return rc;
  if (int rc = e->d_cnpcnt.ensure(sizeof(int64_t) * 2 * chunks.size())) return rc;
  if (int rc = e->d_cnorder.ensure(sizeof(int32_t) * order.size())) return rc;
  if (int rc = e->d_cnchunk.ensure(sizeof(CenChunk) * chunks.size())) return rc;
  if (int rc = e->d_cnoff.ensure(sizeof(int32_t) * ((size_t)G + 1))) return rc;
  if (int rc = e->d_cnw.ensure(sizeof(double) * (size_t)G * V)) return rc;
  if (int rc = e->d_cnact.ensure((size_t)G)) return rc;
  if (int rc = e->d_cnout.ensure(sizeof(double) * (size_t)G * ((size_t)V + 3))) return rc;
  if (int rc = e->d_cncnt.ensure(sizeof(int64_t) * 2 * (size_t)G)) return rc;
  if (!order.empty()) HIP_TRY(hipMemcpyAsync(e->d_cnorder, order.data(), sizeof(int32_t) * order.size(), hipMemcpyHostToDevice, e->stream));
  if (!chunks.empty()) HIP_TRY(hipMemcpyAsync(e->d_cnchunk, chunks.data(), sizeof(CenChunk) * chunks.size(), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_cnoff, plan->chunk_off.data(), sizeof(int32_t) * ((size_t)G + 1), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemsetAsync(e->d_cnout, 0, sizeof(double) * (size_t)G * ((size_t)V + 3), e->stream));
  HIP_TRY(hipMemsetAsync(e->d_cncnt, 0, sizeof(int64_t) * 2 * (size_t)G, e->stream));
  if (S > 0) HIP_TRY(hipMemsetAsync(e->d_cnvalid, 1, (size_t)S, e->stream));
  EventPair& ev = e->cnev;
  if (int rc = ev.record_start(e->stream)) return rc;
  const int64_t items = (int64_t)S * V;
  if (items > 0) {
    hipLaunchKernelGGL(k_census_dosage, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, e->stream, e->d_g, items, V, e->d_cnd, e->d_cnvalid);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = ev.record_stop(e->stream)) return rc;
  std::vector<uint8_t> valid((size_t)S);
  if (S > 0) HIP_TRY(hipMemcpyAsync(valid.data(), e->d_cnvalid, (size_t)S, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));         // (the plan's host vectors go away on return)
  float ms = 0.f;
  if (int rc = ev.elapsed_ms(&ms)) return rc;
  dmx_census_info& inf = e->cen_info;
  std::memset(&inf, 0, sizeof inf);
  inf.dosage_ms = ms; inf.dosage_bytes = (int64_t)dos; inf.partial_bytes = (int64_t)par;
  for (uint8_t x : valid) inf.n_invalid_snps += x == 0;
  inf.n_groups = G; inf.n_chunks = plan->n_chunks; inf.n_cells = B; inf.n_samples = V;
  e->have_cen_info = true;
  return DMX_OK;
}

int census_pass(dmx_engine* e, const CensusPlan& pl, const double* w, const uint8_t* active, double* out) {
  const int32_t G = pl.G, V = pl.V;
  HIP_TRY(hipMemcpyAsync(e->d_cnw, w, sizeof(double) * (size_t)G * V, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_cnact, active, (size_t)G, hipMemcpyHostToDevice, e->stream));
  if (int rc = e->cnev.record_start(e->stream)) return rc;
  if (pl.n_chunks > 0) {
    const size_t lds = sizeof(double) * 2 * kCenWaves * (size_t)((V + 63) & ~63);
    if (lds > 30 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_census_step), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_census_step, dim3((unsigned)((pl.n_chunks + kCenWaves - 1) / kCenWaves)), dim3(64 * kCenWaves), lds, e->stream, e->pv,
                       e->nrd_width, (const double*)e->d_lut, (const double*)e->d_cnd, (const uint8_t*)e->d_cnvalid, V,
                       (const int32_t*)e->d_cnorder, (const CenChunk*)e->d_cnchunk, pl.n_chunks, (const uint8_t*)e->d_cnact,
                       (const double*)e->d_cnw, e->d_cnpart.get(), e->d_cnpcnt.get());
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_census_fold, dim3((unsigned)G), dim3(256), 0, e->stream, (const double*)e->d_cnpart, (const int64_t*)e->d_cnpcnt,
                     (const int32_t*)e->d_cnoff, (const uint8_t*)e->d_cnact, V, e->d_cnout.get(), e->d_cncnt.get());
  HIP_TRY(hipGetLastError());
  if (int rc = e->cnev.record_stop(e->stream)) return rc;
  HIP_TRY(hipMemcpyAsync(out, e->d_cnout, sizeof(double) * (size_t)G * ((size_t)V + 3), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  float ms = 0.f;
  if (int rc = e->cnev.elapsed_ms(&ms)) return rc;
  e->cen_info.kernel_ms = ms; e->cen_info.n_steps += 1;
  return DMX_OK;
}

int census_check_w(const char* fn, const double* w, int32_t G, int32_t V) {
  for (int32_t g = 0; g < G; ++g) {
    double s = 0.0;
    for (int32_t v = 0; v < V; ++v) {
      const double x = w[(size_t)g * V + v];
      if (!(x >= 0.0 && x < INFINITY)) return set_error(DMX_ERR_ARG, "%s: w[%d][%d] = %g is negative or not finite", fn, g, v, x);
      s += x;
    }
    if (!(std::fabs(s - 1.0) <= 1e-12)) return set_error(DMX_ERR_ARG, "%s: row %d of w sums to %.17g, not to 1 within 1e-12", fn, g, s);
  }
  return DMX_OK;
}

}  // namespace

extern "C" int dmx_engine_census_step(dmx_engine* e, const dmx_census_step_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_census_step: null argument");
  CensusPlan pl;
  if (int rc = census_prepare(e, "dmx_engine_census_step", rq->n_cells, rq->group_memory, rq->group, rq->n_groups, rq->n_samples, &pl)) return rc;
  const int32_t G = pl.G, V = pl.V;
  if (!rq->w) return set_error(DMX_ERR_ARG, "dmx_engine_census_step: missing w");
  if (int rc = census_check_w("dmx_engine_census_step", rq->w, G, V)) return rc;
  std::vector<uint8_t> active((size_t)G, 1);
  std::vector<double> out((size_t)G * ((size_t)V + 3));
  if (int rc = census_pass(e, pl, rq->w, active.data(), out.data())) return rc;
  std::vector<int64_t> cnt(2 * (size_t)G);
  HIP_TRY(hipMemcpy(cnt.data(), e->d_cncnt, sizeof(int64_t) * cnt.size(), hipMemcpyDeviceToHost));
  for (int32_t g = 0; g < G; ++g) {
    const double* o = out.data() + (size_t)g * ((size_t)V + 3);
    if (rq->acc) std::memcpy(rq->acc + (size_t)g * V, o, sizeof(double) * (size_t)V);
    if (rq->ll) rq->ll[g] = o[V];
    if (rq->gap) rq->gap[g] = o[V + 1];
    if (rq->n_read) rq->n_read[g] = cnt[2 * (size_t)g];
    if (rq->n_pair) rq->n_pair[g] = cnt[2 * (size_t)g + 1];
  }
  return DMX_OK;
}

extern "C" int dmx_engine_census(dmx_engine* e, const dmx_census_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_census: null argument");
  CensusPlan pl;
  if (int rc = census_prepare(e, "dmx_engine_census", rq->n_cells, rq->group_memory, rq->group, rq->n_groups, rq->n_samples, &pl)) return rc;
  const int32_t G = pl.G, V = pl.V;
  const size_t sv = (size_t)V;
  if (rq->w0) if (int rc = census_check_w("dmx_engine_census", rq->w0, G, V)) return rc;
  const double tol = rq->tol > 0.0 ? rq->tol : 1e-4;
  const int32_t max_steps = rq->max_steps > 0 ? rq->max_steps : 2000;
  const bool accel = rq->accelerate != 0;
  const bool on_support = rq->reserved[0] != 0;    // gap_on_support: the gap's maximum runs over the donors with w0 > 0 only
  std::vector<double> cur((size_t)G * sv), w0(cur.size()), w1(cur.size()), w2(cur.size()), ll1((size_t)G, 0.0), out((size_t)G * (sv + 3));
  if (rq->w0) std::memcpy(cur.data(), rq->w0, sizeof(double) * cur.size());
  else std::fill(cur.begin(), cur.end(), 1.0 / (double)V);
  std::vector<uint8_t> active((size_t)G, 1), support;
  if (on_support) {
    support.resize(cur.size());
    for (size_t i = 0; i < cur.size(); ++i) support[i] = cur[i] > 0.0;
  }
  std::vector<int32_t> phase((size_t)G, 0);
  e->have_census = false;
  e->cn_G = G;
  e->cn_w.assign(cur.size(), 0.0); e->cn_ll.assign((size_t)G, 0.0); e->cn_gap.assign((size_t)G, 0.0);
  e->cn_steps.assign((size_t)G, 0); e->cn_conv.assign((size_t)G, 0);
  e->cn_nread.assign((size_t)G, 0); e->cn_npair.assign((size_t)G, 0);
  int32_t n_active = G;
  bool first = true;
  while (n_active > 0) {
    if (int rc = census_pass(e, pl, cur.data(), active.data(), out.data())) return rc;
    if (first) {
      std::vector<int64_t> cnt(2 * (size_t)G);
      HIP_TRY(hipMemcpy(cnt.data(), e->d_cncnt, sizeof(int64_t) * cnt.size(), hipMemcpyDeviceToHost));
      for (int32_t g = 0; g < G; ++g) { e->cn_nread[(size_t)g] = cnt[2 * (size_t)g]; e->cn_npair[(size_t)g] = cnt[2 * (size_t)g + 1]; }
      first = false;
    }
    for (int32_t g = 0; g < G; ++g) {
      if (!active[(size_t)g]) continue;
      const double* o = out.data() + (size_t)g * (sv + 3);
      double* x = cur.data() + (size_t)g * sv;
      const double ll = o[V], N = o[V + 2];
      double gap = o[V + 1];
      if (on_support && N > 0.0) {                 // EM and SQUAREM keep zeros at zero: the constrained problem's own duality gap
        double mx = 0.0;
        for (size_t v = 0; v < sv; ++v) if (support[(size_t)g * sv + v]) mx = std::fmax(mx, o[v]);
        gap = N * (mx / N - 1.0);
      }
      const int32_t steps = ++e->cn_steps[(size_t)g];
      const bool empty = !(N > 0.0), conv = empty || (std::isfinite(ll) && gap <= tol);
      if (conv || steps >= max_steps) {
        std::memcpy(e->cn_w.data() + (size_t)g * sv, x, sizeof(double) * sv);
        e->cn_ll[(size_t)g] = empty ? 0.0 : ll; e->cn_gap[(size_t)g] = empty ? 0.0 : gap; e->cn_conv[(size_t)g] = conv ? 1 : 0;
        active[(size_t)g] = 0; n_active -= 1;
        continue;
      }
      double* a0 = w0.data() + (size_t)g * sv; double* a1 = w1.data() + (size_t)g * sv; double* a2 = w2.data() + (size_t)g * sv;
      if (!accel) {
        for (size_t v = 0; v < sv; ++v) x[v] = x[v] * o[v] / N;
      } else if (phase[(size_t)g] == 0) {
        for (size_t v = 0; v < sv; ++v) { a0[v] = x[v]; a1[v] = x[v] * o[v] / N; x[v] = a1[v]; }
        phase[(size_t)g] = 1;
      } else if (phase[(size_t)g] == 1) {
        ll1[(size_t)g] = ll;
        double rr = 0.0, uu = 0.0;
        for (size_t v = 0; v < sv; ++v) {
          a2[v] = x[v] * o[v] / N;
          const double r = a1[v] - a0[v], u = (a2[v] - a1[v]) - r;
          rr += r * r; uu += u * u;
        }
        double a = uu > 0.0 ? -std::sqrt(rr) / std::sqrt(uu) : -1.0;
        if (!(a <= -1.0) || !std::isfinite(a)) a = -1.0;
        for (;;) {
          bool neg = false;
          for (size_t v = 0; v < sv; ++v) {
            const double r = a1[v] - a0[v], u = (a2[v] - a1[v]) - r;
            x[v] = (a0[v] - 2.0 * a * r) + a * a * u;
            neg = neg || x[v] < 0.0;
          }
          if (!neg || a == -1.0) break;
          a = 0.5 * (a - 1.0);
          if (a > -1.0 - 1e-9) a = -1.0;
        }
        if (a == -1.0) std::memcpy(x, a2, sizeof(double) * sv);
        double s = 0.0;
        for (size_t v = 0; v < sv; ++v) { if (!(x[v] > 0.0)) x[v] = 0.0; s += x[v]; }
        for (size_t v = 0; v < sv; ++v) x[v] /= s;
        phase[(size_t)g] = 2;
      } else {
        if (!std::isfinite(ll) || ll < ll1[(size_t)g]) std::memcpy(x, a2, sizeof(double) * sv);
        else for (size_t v = 0; v < sv; ++v) x[v] = x[v] * o[v] / N;
        phase[(size_t)g] = 0;
      }
    }
  }
  e->have_census = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_census(dmx_engine* e, double* w, double* ll, double* gap, int32_t* n_steps, int32_t* converged, int64_t* n_read,
                                     int64_t* n_pair) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_census: null engine");
  if (!e->have_census) return set_error(DMX_ERR_STATE, "dmx_engine_get_census: no census on the staged pileup (dmx_engine_census first)");
  const size_t G = (size_t)e->cn_G;
  if (w) std::memcpy(w, e->cn_w.data(), sizeof(double) * e->cn_w.size());
  if (ll) std::memcpy(ll, e->cn_ll.data(), sizeof(double) * G);
  if (gap) std::memcpy(gap, e->cn_gap.data(), sizeof(double) * G);
  if (n_steps) std::memcpy(n_steps, e->cn_steps.data(), sizeof(int32_t) * G);
  if (converged) std::memcpy(converged, e->cn_conv.data(), sizeof(int32_t) * G);
  if (n_read) std::memcpy(n_read, e->cn_nread.data(), sizeof(int64_t) * G);
  if (n_pair) std::memcpy(n_pair, e->cn_npair.data(), sizeof(int64_t) * G);
  return DMX_OK;
}

extern "C" int dmx_engine_census_info(dmx_engine* e, dmx_census_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_census_info: null argument");
  if (!e->have_cen_info) return set_error(DMX_ERR_STATE, "dmx_engine_census_info: no census pass on the staged pileup (dmx_engine_census_step or dmx_engine_census first)");
  *out = e->cen_info;
  return DMX_OK;
}

// Census uncertainty: census_prepare's plan and dosage table, one census_pass at w for acc, LL and the counts
// (so they carry dmx_engine_census_step's bits), then k_census_fisher and k_census_fisher_fold into buffers of this call's own.
extern "C" int dmx_engine_census_fisher(dmx_engine* e, const dmx_census_fisher_request* rq) {
  const char* fn = "dmx_engine_census_fisher";
  if (!e || !rq) return set_error(DMX_ERR_ARG, "%s: null argument", fn);
  const dmx_census_info keep_info = e->cen_info;   // the census calls' own info survives this call
  const bool keep_have = e->have_cen_info;
  struct Restore {
    dmx_engine* e; const dmx_census_info& i; bool h;
    ~Restore() { e->cen_info = i; e->have_cen_info = h; }
  } restore{e, keep_info, keep_have};
  CensusPlan pl;
  if (int rc = census_prepare(e, fn, rq->n_cells, rq->group_memory, rq->group, rq->n_groups, rq->n_samples, &pl)) return rc;
  const int32_t G = pl.G, V = pl.V, B = e->pv.B;
  if (V > kFisMaxV) return set_error(DMX_ERR_ARG, "%s: %d samples, at most %d", fn, V, kFisMaxV);
  if (!rq->w) return set_error(DMX_ERR_ARG, "%s: missing w", fn);
  if (int rc = census_check_w(fn, rq->w, G, V)) return rc;
  const size_t E = (size_t)V * ((size_t)V + 1) / 2;
  const int32_t n_blocks = (int32_t)((E + kFisBlock - 1) / kFisBlock);
  const int64_t units = (int64_t)pl.n_chunks * n_blocks;
  if (units > INT32_MAX - kCenWaves) return set_error(DMX_ERR_ARG, "%s: %d chunks x %d entry blocks", fn, pl.n_chunks, n_blocks);
  const size_t par = sizeof(double) * (size_t)pl.n_chunks * E, hb = sizeof(double) * (size_t)G * V * V, sb = sizeof(double) * (size_t)B * V;
  const size_t nbb = sizeof(int64_t) * (size_t)B;
  size_t free_b = 0, total_b = 0, need = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (par > e->d_fspart.cap()) need += par + par / 16;
  if (hb > e->d_fsH.cap()) need += hb + hb / 16;
  if (sb > e->d_fsscore.cap()) need += sb + sb / 16;
  if (nbb > e->d_fsnb.cap()) need += nbb + nbb / 16;
  if (need > free_b)
    return set_error(DMX_ERR_NOMEM, "%s: %d chunk partials of %zu entries, H and the score rows need %zu bytes, %zu are free", fn, pl.n_chunks, E, need, free_b);
  if (int rc = e->d_fspart.ensure(par)) return rc;
  if (int rc = e->d_fsH.ensure(hb)) return rc;
  if (int rc = e->d_fsscore.ensure(sb)) return rc;
  if (int rc = e->d_fsnb.ensure(nbb)) return rc;
  std::vector<uint8_t> active((size_t)G, 1);
  std::vector<double> out((size_t)G * ((size_t)V + 3));
  if (int rc = census_pass(e, pl, rq->w, active.data(), out.data())) return rc;      // (leaves w[G][V] in d_cnw)
  std::vector<int64_t> cnt(2 * (size_t)G);
  HIP_TRY(hipMemcpyAsync(cnt.data(), e->d_cncnt, sizeof(int64_t) * cnt.size(), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemsetAsync(e->d_fsH, 0, hb, e->stream));
  if (sb) HIP_TRY(hipMemsetAsync(e->d_fsscore, 0, sb, e->stream));
  if (B > 0) HIP_TRY(hipMemsetAsync(e->d_fsnb, 0, nbb, e->stream));
  if (int rc = e->fsev.record_start(e->stream)) return rc;
  if (units > 0) {
    hipLaunchKernelGGL(k_census_fisher, dim3((unsigned)((units + kCenWaves - 1) / kCenWaves)), dim3(64 * kCenWaves), 0, e->stream, e->pv,
                       e->nrd_width, (const double*)e->d_lut, (const double*)e->d_cnd, (const uint8_t*)e->d_cnvalid, V,
                       (const int32_t*)e->d_cnorder, (const CenChunk*)e->d_cnchunk, pl.n_chunks, n_blocks, (const double*)e->d_cnw,
                       e->d_fspart.get(), e->d_fsscore.get(), e->d_fsnb.get());
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_census_fisher_fold, dim3((unsigned)G, (unsigned)((E + 255) / 256)), dim3(256), 0, e->stream, (const double*)e->d_fspart,
                     (const int32_t*)e->d_cnoff, V, e->d_fsH.get());
  HIP_TRY(hipGetLastError());
  if (int rc = e->fsev.record_stop(e->stream)) return rc;
  if (rq->H) HIP_TRY(hipMemcpyAsync(rq->H, e->d_fsH, hb, hipMemcpyDeviceToHost, e->stream));
  if (rq->score && sb) HIP_TRY(hipMemcpyAsync(rq->score, e->d_fsscore, sb, hipMemcpyDeviceToHost, e->stream));
  if (rq->n_read_b && B > 0) HIP_TRY(hipMemcpyAsync(rq->n_read_b, e->d_fsnb, nbb, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  float ms = 0.f;
  if (int rc = e->fsev.elapsed_ms(&ms)) return rc;
  for (int32_t g = 0; g < G; ++g) {
    const double* o = out.data() + (size_t)g * ((size_t)V + 3);
    if (rq->acc) std::memcpy(rq->acc + (size_t)g * V, o, sizeof(double) * (size_t)V);
    if (rq->ll) rq->ll[g] = o[V];
    if (rq->n_read) rq->n_read[g] = cnt[2 * (size_t)g];
    if (rq->n_pair) rq->n_pair[g] = cnt[2 * (size_t)g + 1];
  }
  dmx_census_fisher_info& inf = e->fis_info;
  std::memset(&inf, 0, sizeof inf);
  inf.kernel_ms = ms; inf.partial_bytes = (int64_t)par;
  inf.n_groups = G; inf.n_chunks = pl.n_chunks; inf.n_blocks = n_blocks; inf.n_entries = (int32_t)E; inf.n_cells = B; inf.n_samples = V;
  e->have_fis_info = true;
  return DMX_OK;
}

extern "C" int dmx_engine_census_fisher_info(dmx_engine* e, dmx_census_fisher_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_census_fisher_info: null argument");
  if (!e->have_fis_info) return set_error(DMX_ERR_STATE, "dmx_engine_census_fisher_info: no call on the staged pileup (dmx_engine_census_fisher first)");
  *out = e->fis_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
namespace {
template <int WHICH>   // 0: dmx_log (128 bins; the singlet kernels), 2: dmx_log2 (256 bins; the doublet kernels), 3: dmx_log2_lite, 4: dmx_log2_lite32 (FAST)
__global__ void k_debug_log(const double* __restrict__ x, double* __restrict__ y, int64_t n, const double* __restrict__ tab) {
  __shared__ double s_log[DMX_LOG2_TABLE_DOUBLES];
  for (int i = threadIdx.x; i < (WHICH == 4 ? DMX_LOG32_TABLE_DOUBLES : WHICH >= 2 ? DMX_LOG2_TABLE_DOUBLES : DMX_LOG_TABLE_DOUBLES); i += blockDim.x) s_log[i] = tab[i];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = WHICH == 4 ? dmx_log2_lite32(x[i], s_log, dmx_log32_pins())
                   : WHICH == 3 ? dmx_log2_lite(x[i], s_log, dmx_log_pins()) : (WHICH == 2 ? dmx_log2_fast(x[i], s_log) : dmx_log_fast(x[i], s_log));
    y[i] = dmx_log_is_special(x[i]) ? log(x[i]) : v;
  }
}
// a mirrored pair per lane through the device functions the STRICT unordered-pair kernels call, their wave-uniform guard test included (normal positive arguments)
__global__ void k_debug_log2_mirror(const double* __restrict__ x, const double* __restrict__ xm, double* __restrict__ y, double* __restrict__ ym, int64_t n,
                                    const double* __restrict__ tab) {
  __shared__ double s_log[DMX_LOG2_TABLE_DOUBLES];
  for (int i = threadIdx.x; i < DMX_LOG2_TABLE_DOUBLES; i += blockDim.x) s_log[i] = tab[i];
  __syncthreads();
  const DmxLogPins lk = dmx_log_pins();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const DmxLog2MirrorReq m = dmx_log2_request_mirror_fast(x[i], xm[i], s_log);
    double vm;
    const double v = dmx_log2_finish_mirror_pinned(m, lk, &vm);
    if (dmx_log2_mirror_any_redo<false>(m.guard)) vm = dmx_log2_mirror_settle<false>(m.guard, m, vm, s_log, lk);
    y[i] = v;
    ym[i] = vm;
  }
}
}  // namespace

namespace {
__global__ void k_debug_div(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ q, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    q[i] = div_by(a[i], b[i], rcp_refined(b[i]));
}
}  // namespace

namespace {
// log() ceiling of the device: every lane evaluates `iters` logs of register-resident arguments spread over (0.01, 1] (the
// range likelihood terms live in), four independent streams per lane so the issue rate, not the latency, is measured.
// WHICH = 0: dmx_log (the singlet kernels), 1: ocml log(), 2: dmx_log2 (the doublet kernels).
template <int WHICH>
__global__ __launch_bounds__(256) void k_log_rate(int iters, const double* __restrict__ tab, double* __restrict__ sink) {
  __shared__ double s_log[DMX_LOG2_TABLE_DOUBLES];
  for (int i = threadIdx.x; i < (WHICH == 2 ? DMX_LOG2_TABLE_DOUBLES : DMX_LOG_TABLE_DOUBLES); i += blockDim.x) s_log[i] = tab[i];
  __syncthreads();
  const double x0 = 0.01 + 0.9 * ((threadIdx.x * 37 + blockIdx.x * 11) % 1024) / 1024.0;
  double x[4] = {x0, x0 * 0.75, x0 * 0.5, x0 * 0.31}, acc[4] = {0.0, 0.0, 0.0, 0.0};
  const double dx = 1.0 / (1024.0 * 1024.0);
  for (int i = 0; i < iters; i += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc[u] += WHICH == 0 ? dmx_log(x[u], s_log) : (WHICH == 2 ? dmx_log2_fast(x[u], s_log) : log(x[u]));
      x[u] += dx;
    }
  }
  sink[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
}
}  // namespace

extern "C" int dmx_debug_log_rate(int32_t which, int32_t iters, int32_t device, double* logs_per_second) {
  if (which < 0 || which > 2 || iters < 4 || !logs_per_second) return set_error(DMX_ERR_ARG, "dmx_debug_log_rate: bad arguments");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return set_error(DMX_ERR_NOGPU, "dmx_debug_log_rate: no such HIP device");
  HIP_TRY(hipSetDevice(device));
  const int blocks = 256 * 8, threads = 256;                  // 8 workgroups (32 wavefronts) per CU
  DevBuf<double> dt, ds;
  if (int rc = dt.alloc(sizeof(double) * DMX_LOG2_TABLE_DOUBLES)) return rc;
  if (int rc = ds.alloc(sizeof(double) * (size_t)blocks * threads)) return rc;
  if (which == 2) HIP_TRY(hipMemcpy(dt, dmx_log2_table_host, sizeof(double) * DMX_LOG2_TABLE_DOUBLES, hipMemcpyHostToDevice));
  else HIP_TRY(hipMemcpy(dt, dmx_log_table_host, sizeof(double) * DMX_LOG_TABLE_DOUBLES, hipMemcpyHostToDevice));
  EventPair ev;
  iters &= ~3;
  float best = 1e30f;
  for (int rep = 0; rep < 4; ++rep) {                          // first pass warms up; keep the fastest
    if (int rc = ev.record_start(0)) return rc;
    if (which == 0) hipLaunchKernelGGL((k_log_rate<0>), dim3(blocks), dim3(threads), 0, 0, iters, dt, ds);
    else if (which == 2) hipLaunchKernelGGL((k_log_rate<2>), dim3(blocks), dim3(threads), 0, 0, iters, dt, ds);
    else            hipLaunchKernelGGL((k_log_rate<1>), dim3(blocks), dim3(threads), 0, 0, iters, dt, ds);
    if (int rc = ev.record_stop(0)) return rc;
    HIP_TRY(hipEventSynchronize(ev.stop));
    HIP_TRY(hipGetLastError());
    float ms = 0.f;
    if (int rc = ev.elapsed_ms(&ms)) return rc;
    if (rep > 0 && ms < best) best = ms;
  }
  *logs_per_second = (double)blocks * threads * iters / (best * 1e-3);
  return DMX_OK;
}

extern "C" int dmx_debug_device_div(const double* a, const double* b, double* q, int64_t n, int32_t device) {
  if (!a || !b || !q || n < 0) return set_error(DMX_ERR_ARG, "dmx_debug_device_div: bad arguments");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return set_error(DMX_ERR_NOGPU, "dmx_debug_device_div: no such HIP device");
  HIP_TRY(hipSetDevice(device));
  DevBuf<double> da, db, dq;
  const size_t bytes = std::max<size_t>(sizeof(double) * (size_t)n, 16);
  for (DevBuf<double>* d : {&da, &db, &dq}) if (int rc = d->alloc(bytes)) return rc;
  HIP_TRY(hipMemcpy(da, a, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(db, b, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_debug_div, dim3(1024), dim3(256), 0, 0, da, db, dq, n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(q, dq, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return DMX_OK;
}

namespace {
int debug_device_log(int which, const double* x, double* y, int64_t n, int32_t device) {
  if (!x || !y || n < 0) return set_error(DMX_ERR_ARG, "dmx_debug_device_log: bad arguments");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return set_error(DMX_ERR_NOGPU, "dmx_debug_device_log: no such HIP device");
  HIP_TRY(hipSetDevice(device));
  DevBuf<double> dx, dy, dt;
  if (int rc = dx.alloc(std::max<size_t>(sizeof(double) * (size_t)n, 16))) return rc;
  if (int rc = dy.alloc(std::max<size_t>(sizeof(double) * (size_t)n, 16))) return rc;
  if (int rc = dt.alloc(sizeof(double) * DMX_LOG2_TABLE_DOUBLES)) return rc;
  HIP_TRY(hipMemcpy(dx, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  if (which == 4) HIP_TRY(hipMemcpy(dt, dmx_log32_table_host, sizeof(double) * DMX_LOG32_TABLE_DOUBLES, hipMemcpyHostToDevice));
  else if (which >= 2) HIP_TRY(hipMemcpy(dt, dmx_log2_table_host, sizeof(double) * DMX_LOG2_TABLE_DOUBLES, hipMemcpyHostToDevice));
  else HIP_TRY(hipMemcpy(dt, dmx_log_table_host, sizeof(double) * DMX_LOG_TABLE_DOUBLES, hipMemcpyHostToDevice));
  if (which == 4) hipLaunchKernelGGL((k_debug_log<4>), dim3(1024), dim3(256), 0, 0, dx, dy, n, dt);
  else if (which == 3) hipLaunchKernelGGL((k_debug_log<3>), dim3(1024), dim3(256), 0, 0, dx, dy, n, dt);
  else if (which == 2) hipLaunchKernelGGL((k_debug_log<2>), dim3(1024), dim3(256), 0, 0, dx, dy, n, dt);
  else hipLaunchKernelGGL((k_debug_log<0>), dim3(1024), dim3(256), 0, 0, dx, dy, n, dt);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(y, dy, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return DMX_OK;
}
}  // namespace
extern "C" int dmx_debug_device_log(const double* x, double* y, int64_t n, int32_t device) { return debug_device_log(0, x, y, n, device); }
extern "C" int dmx_debug_device_log2(const double* x, double* y, int64_t n, int32_t device) { return debug_device_log(2, x, y, n, device); }
extern "C" int dmx_debug_device_log2_lite(const double* x, double* y, int64_t n, int32_t device) { return debug_device_log(3, x, y, n, device); }
extern "C" int dmx_debug_device_log2_lite32(const double* x, double* y, int64_t n, int32_t device) { return debug_device_log(4, x, y, n, device); }
extern "C" int dmx_debug_device_log2_mirror(const double* x, const double* xm, double* y, double* ym, int64_t n, int32_t device) {
  if (!x || !xm || !y || !ym || n < 0) return set_error(DMX_ERR_ARG, "dmx_debug_device_log2_mirror: bad arguments");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return set_error(DMX_ERR_NOGPU, "dmx_debug_device_log2_mirror: no such HIP device");
  HIP_TRY(hipSetDevice(device));
  DevBuf<double> dx, dxm, dy, dym, dt;
  const size_t bytes = std::max<size_t>(sizeof(double) * (size_t)n, 16);
  for (DevBuf<double>* d : {&dx, &dxm, &dy, &dym}) if (int rc = d->alloc(bytes)) return rc;
  if (int rc = dt.alloc(sizeof(double) * DMX_LOG2_TABLE_DOUBLES)) return rc;
  HIP_TRY(hipMemcpy(dx, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dxm, xm, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dt, dmx_log2_table_host, sizeof(double) * DMX_LOG2_TABLE_DOUBLES, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_debug_log2_mirror, dim3(1024), dim3(256), 0, 0, dx, dxm, dy, dym, n, dt);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(y, dy, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ym, dym, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// (ABI 8) `.pair` rows formatted on the device (csrc/dmx_format.hpp)
#include "dmx_format.hpp"

struct dmx_pair_text {
  int device = 0;
  DevBuf<char> d_text;
  int64_t n_bytes = 0;
  std::vector<int64_t> cell_off;
  std::vector<uint8_t> cell_flag;
  std::vector<dmx_pair_patch> patches;
  std::vector<dmx_pair_scalars> scal;
  double format_ms = 0.0;
};

// The limits of the device `.pair` path (dmx.h) in one place: the row map's fields hold 12 bits of a sample index and 8 of an alpha index, and a
// chunk of 256 rows has to fit k_pair_write's LDS buffer.  dmx_engine_format_pair refuses what does not fit; dmx_demuxlet_run asks first and
// leaves such a job to the host formatter.  Returns nullptr when the path applies, else what is in the way.
static const char* pair_device_limit(int32_t V, int32_t A, size_t bc_max, size_t sm_max, size_t al_max, size_t* max_row_out) {
  const size_t max_row = bc_max + 1 + 2 * sm_max + 1 + al_max + 20 + 1 + 12 + 1;   // "%s\t%s\t%s" "\t%.3lf\t" "%.5lf" "\t" "%.5lg" "\n"
  if (max_row_out) *max_row_out = max_row;
  if (V > 4095 || A > 255) return "samples x alphas exceed the row map's fields";
  if (max_row > (size_t)150 * 1024 / dmx_fmt::kFmtThreads) return "rows do not fit the kernel's buffer";
  return nullptr;
}
// "\t%.3lf\t" of one alpha, the reference's own conversion (:776,:788); false when it does not print
static bool pair_alpha_text(double alpha, std::string* out) {
  char buf[400];
  const int n = std::snprintf(buf, sizeof buf, "\t%.3lf\t", alpha);
  if (n < 0 || (size_t)n >= sizeof buf) return false;
  out->assign(buf, (size_t)n);
  return true;
}

extern "C" void dmx_pair_text_free(dmx_pair_text* t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  delete t;
}

extern "C" int dmx_pair_text_get_info(const dmx_pair_text* t, dmx_pair_text_info* out) {
  if (!t || !out) return set_error(DMX_ERR_ARG, "dmx_pair_text_get_info: null argument");
  out->n_bytes = t->n_bytes; out->n_out = (int32_t)t->cell_flag.size(); out->n_patches = (int32_t)t->patches.size();
  out->cell_off = t->cell_off.data(); out->cell_flag = t->cell_flag.data(); out->patches = t->patches.data(); out->format_ms = t->format_ms;
  return DMX_OK;
}

extern "C" int dmx_pair_text_get_scalars(const dmx_pair_text* t, const dmx_pair_scalars** out) {
  if (!t || !out) return set_error(DMX_ERR_ARG, "dmx_pair_text_get_scalars: null argument");
  *out = t->scal.data();
  return DMX_OK;
}

extern "C" int dmx_pair_text_read(dmx_pair_text* t, int64_t offset, int64_t n, void* dst) {
  if (!t || offset < 0 || n < 0 || offset + n > t->n_bytes || (n && !dst)) return set_error(DMX_ERR_ARG, "dmx_pair_text_read: bad arguments");
  if (!n) return DMX_OK;
  HIP_TRY(hipSetDevice(t->device));
  HIP_TRY(hipMemcpy(dst, t->d_text + offset, (size_t)n, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_format_pair(dmx_engine* e, const dmx_pair_request* rq, dmx_pair_text** out) {
  if (!e || !rq || !out || rq->n_out < 0 || (rq->n_out && (!rq->cells || !rq->barcodes)) || !rq->sample_ids)
    return set_error(DMX_ERR_ARG, "dmx_engine_format_pair: null argument");
  if (!e->have_grid) return set_error(DMX_ERR_STATE, "dmx_engine_format_pair: run_doublet has not been called");
  const int32_t V = e->V, A = e->A, n_out = rq->n_out;
  if (pair_device_limit(V, A, 0, 0, 0, nullptr)) return set_error(DMX_ERR_ARG, "dmx_engine_format_pair: %d samples x %d alphas exceed the row map's fields", V, A);
  for (int32_t i = 0; i < n_out; ++i) {
    if (rq->ovr && rq->ovr[i].n >= 0 && (rq->ovr[i].a < 0 || rq->ovr[i].a >= V || rq->ovr[i].b < 0 || rq->ovr[i].b >= V || rq->ovr[i].n >= A))
      return set_error(DMX_ERR_ARG, "dmx_engine_format_pair: ovr[%d] = (%d, %d, %d) is not an entry of the grid", i, rq->ovr[i].a, rq->ovr[i].b, rq->ovr[i].n);
    if (rq->cells[i] < 0 || rq->cells[i] >= e->pv.B) return set_error(DMX_ERR_ARG, "dmx_engine_format_pair: cell %d out of range (0..%d)", rq->cells[i], e->pv.B - 1);
    if (!rq->barcodes[i]) return set_error(DMX_ERR_ARG, "dmx_engine_format_pair: barcodes[%d] is null", i);
  }
  for (int32_t j = 0; j < V; ++j) if (!rq->sample_ids[j]) return set_error(DMX_ERR_ARG, "dmx_engine_format_pair: sample_ids[%d] is null", j);
  HIP_TRY(hipSetDevice(e->device));
  // ---- host-side tables: the rows of one barcode in print order (:772-797), the strings, "\t%.3lf\t" of every alpha, powers of ten
  std::vector<uint32_t> rowmap;
  for (int32_t j = 0; j < V; ++j) {
    rowmap.push_back(((uint32_t)j << 20) | ((uint32_t)j << 8));                                  // :774-781 the singlet row (SM1 = SM2 = j, alpha[0])
    for (int32_t k = 0; k < V; ++k)
      for (int32_t a = 1; a < A; ++a) {
        if (j == k) continue;
        if (j > k && e->alpha[(size_t)a] == 0.5) continue;                                       // :785
        rowmap.push_back(((uint32_t)j << 20) | ((uint32_t)k << 8) | (uint32_t)a);
      }
  }
  auto pool_of = [](const char* const* strs, int32_t n, std::string* pool, std::vector<uint32_t>* off, size_t* longest) -> bool {
    off->assign(1, 0u);
    for (int32_t i = 0; i < n; ++i) {
      const size_t len = std::strlen(strs[i]);
      if (pool->size() + len >= 0xFFFFFFF0ull) return false;
      pool->append(strs[i], len);
      off->push_back((uint32_t)pool->size());
      *longest = std::max(*longest, len);
    }
    return true;
  };
  std::string bc_pool, sm_pool, al_pool;
  std::vector<uint32_t> bc_off, sm_off, al_off(1, 0u);
  size_t bc_max = 0, sm_max = 0, al_max = 0;
  if (!pool_of(rq->barcodes, n_out, &bc_pool, &bc_off, &bc_max) || !pool_of(rq->sample_ids, V, &sm_pool, &sm_off, &sm_max))
    return set_error(DMX_ERR_ARG, "dmx_engine_format_pair: more than 4 GB of barcode text");
  for (int32_t a = 0; a < A; ++a) {
    std::string txt;
    if (!pair_alpha_text(e->alpha[(size_t)a], &txt)) return set_error(DMX_ERR_ARG, "dmx_engine_format_pair: alpha[%d] does not print", a);
    al_pool.append(txt); al_off.push_back((uint32_t)al_pool.size()); al_max = std::max(al_max, txt.size());
  }
  size_t max_row = 0;
  if (pair_device_limit(V, A, bc_max, sm_max, al_max, &max_row))
    return set_error(DMX_ERR_ARG, "dmx_engine_format_pair: rows of up to %zu bytes do not fit the kernel's buffer", max_row);
  const size_t lds = (size_t)dmx_fmt::kFmtThreads * max_row;
  std::vector<double> pow10(310);
  for (int n = 0; n < 310; ++n) { char b[16]; std::snprintf(b, sizeof b, "1e%d", n); pow10[(size_t)n] = std::strtod(b, nullptr); }   // correctly rounded
  // ---- device copies (small; per call)
  std::deque<DevBuf<void>> dev;
  hipStream_t st = e->stream;
  auto up = [&](const void* src, size_t bytes, void** d) -> int {
    dev.emplace_back();
    if (int rc = dev.back().alloc(std::max<size_t>(bytes, 16))) return rc;
    *d = dev.back();
    if (bytes && src) HIP_TRY(hipMemcpyAsync(*d, src, bytes, hipMemcpyHostToDevice, st));
    return DMX_OK;
  };
  dmx_fmt::Ctx c{};
  c.grid = e->d_grid; c.summ = e->d_sum; c.alpha = e->d_alpha; c.prior = e->prior; c.V = V; c.A = A; c.n_out = n_out; c.n_rows = (int32_t)rowmap.size();
  c.max_row = (int32_t)max_row;
  void* d = nullptr;
  if (int rc = up(rq->cells, sizeof(int32_t) * (size_t)n_out, &d)) return rc; c.cells = (const int32_t*)d;
  if (rq->host_rows) { if (int rc = up(rq->host_rows, (size_t)n_out, &d)) return rc; c.host_rows = (const uint8_t*)d; }
  if (rq->ovr) { if (int rc = up(rq->ovr, sizeof(dmx_pair_override) * (size_t)n_out, &d)) return rc; c.ovr = (const dmx_pair_override*)d; }
  if (int rc = up(rowmap.data(), sizeof(uint32_t) * rowmap.size(), &d)) return rc; c.rowmap = (const uint32_t*)d;
  if (int rc = up(bc_pool.data(), bc_pool.size(), &d)) return rc; c.bc_pool = (const char*)d;
  if (int rc = up(bc_off.data(), sizeof(uint32_t) * bc_off.size(), &d)) return rc; c.bc_off = (const uint32_t*)d;
  if (int rc = up(sm_pool.data(), sm_pool.size(), &d)) return rc; c.sm_pool = (const char*)d;
  if (int rc = up(sm_off.data(), sizeof(uint32_t) * sm_off.size(), &d)) return rc; c.sm_off = (const uint32_t*)d;
  if (int rc = up(al_pool.data(), al_pool.size(), &d)) return rc; c.al_pool = (const char*)d;
  if (int rc = up(al_off.data(), sizeof(uint32_t) * al_off.size(), &d)) return rc; c.al_off = (const uint32_t*)d;
  if (int rc = up(pow10.data(), sizeof(double) * pow10.size(), &d)) return rc; c.pow10 = (const double*)d;
  int64_t* d_len = nullptr; uint32_t* d_np = nullptr; int64_t* d_off = nullptr; uint32_t* d_poff = nullptr; uint8_t* d_flag = nullptr;
  dmx_pair_scalars* d_scal = nullptr;
  if (int rc = up(nullptr, sizeof(dmx_pair_scalars) * (size_t)std::max(n_out, 1), (void**)&d_scal)) return rc;
  c.scal = d_scal;
  if (int rc = up(nullptr, sizeof(int64_t) * (size_t)std::max(n_out, 1), (void**)&d_len)) return rc;
  if (int rc = up(nullptr, sizeof(uint32_t) * (size_t)std::max(n_out, 1), (void**)&d_np)) return rc;
  if (int rc = up(nullptr, sizeof(int64_t) * ((size_t)n_out + 1), (void**)&d_off)) return rc;
  if (int rc = up(nullptr, sizeof(uint32_t) * ((size_t)n_out + 1), (void**)&d_poff)) return rc;
  if (int rc = up(nullptr, (size_t)std::max(n_out, 1), (void**)&d_flag)) return rc;
  c.cell_len = d_len; c.cell_npatch = d_np; c.cell_off = d_off; c.cell_poff = d_poff; c.cell_flag = d_flag;
  std::unique_ptr<dmx_pair_text, void (*)(dmx_pair_text*)> t(new (std::nothrow) dmx_pair_text, dmx_pair_text_free);
  if (!t) return set_error(DMX_ERR_NOMEM, "dmx_engine_format_pair: out of memory");
  t->device = e->device;
  t->cell_off.assign((size_t)n_out + 1, 0);
  t->cell_flag.assign((size_t)n_out, 0);
  t->scal.assign((size_t)std::max(n_out, 1), dmx_pair_scalars{0.0, 0.0, 0.0});
  EventPair ev;
  if (n_out > 0) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&dmx_fmt::k_pair_write), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (int rc = ev.record_start(st)) return rc;
    hipLaunchKernelGGL(dmx_fmt::k_pair_lengths, dim3((unsigned)n_out), dim3(dmx_fmt::kFmtThreads), 0, st, c);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(dmx_fmt::k_pair_scan, dim3(1), dim3(1024), 0, st, d_len, d_np, n_out, d_off, d_poff);
    HIP_TRY(hipGetLastError());
    uint32_t n_patch = 0;
    HIP_TRY(hipMemcpyAsync(t->cell_off.data(), d_off, sizeof(int64_t) * ((size_t)n_out + 1), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&n_patch, d_poff + n_out, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(t->cell_flag.data(), d_flag, (size_t)n_out, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    t->n_bytes = t->cell_off[(size_t)n_out];
    t->patches.resize(n_patch);
    if (int rc = t->d_text.alloc((size_t)std::max<int64_t>(t->n_bytes, 16))) return rc;
    dmx_pair_patch* d_patch = nullptr;
    if (int rc = up(nullptr, sizeof(dmx_pair_patch) * (size_t)std::max<uint32_t>(n_patch, 1), (void**)&d_patch)) return rc;
    c.text = t->d_text; c.patches = d_patch;
    hipLaunchKernelGGL(dmx_fmt::k_pair_write, dim3((unsigned)n_out), dim3(dmx_fmt::kFmtThreads), lds, st, c);
    HIP_TRY(hipGetLastError());
    if (int rc = ev.record_stop(st)) return rc;
    if (n_patch) HIP_TRY(hipMemcpyAsync(t->patches.data(), d_patch, sizeof(dmx_pair_patch) * n_patch, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(t->scal.data(), d_scal, sizeof(dmx_pair_scalars) * (size_t)n_out, hipMemcpyDeviceToHost, st));   // (after the timed kernels, with the patches)
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    if (int rc = ev.elapsed_ms(&ms)) return rc;
    t->format_ms = ms;
  }
  *out = t.release();
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// cmd_cram_demuxlet.cpp:390-881 in one call: store (or a frozen pileup) + genotype matrix in, four text files out.
extern "C" int dmx_demuxlet_run(const dmx_job* job) {
  if (!job || (!job->store && !(job->pileup && job->barcodes)) || !job->g || !job->sample_ids || !job->alpha || !job->out_prefix)
    return set_error(DMX_ERR_ARG, "dmx_demuxlet_run: null argument");
  using clk = std::chrono::steady_clock;
  auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
  const clk::time_point t_begin = clk::now();
  dmx_job_timing tm{};
  dmx_pileup pl;
  if (job->store) { if (int rc = dmx_store_freeze(job->store, &pl)) return rc; }
  else {
    pl = *job->pileup;
    if (pl.memory != DMX_MEM_HOST && pl.memory != DMX_MEM_DEVICE) return set_error(DMX_ERR_ARG, "dmx_demuxlet_run: job->pileup.memory %d", pl.memory);
    if (!pl.rd_totl || !pl.rd_pass || !pl.rd_uniq) return set_error(DMX_ERR_ARG, "dmx_demuxlet_run: job->pileup needs the per-cell read counters");
    // everything this function itself indexes before the engine's own checks run
    if (pl.n_cells < 0 || pl.n_snps < 0 || pl.n_pairs < 0 || pl.n_reads < 0) return set_error(DMX_ERR_ARG, "dmx_demuxlet_run: job->pileup has a negative size");
    if (!pl.cell_pair_off || !pl.cell_read_off) return set_error(DMX_ERR_ARG, "dmx_demuxlet_run: job->pileup needs cell_pair_off and cell_read_off");
    for (int32_t c = 0; c < pl.n_cells; ++c) if (!job->barcodes[c]) return set_error(DMX_ERR_ARG, "dmx_demuxlet_run: barcodes[%d] is null", c);
  }
  // A DEVICE-resident pileup (dmx_pileup.memory == DMX_MEM_DEVICE: the five arrays live in the HBM of job->device; counters and barcodes are
  // host memory as always): nothing is sliced or copied on the host.  Its two offset arrays come to the host once (range cuts, N.SNP);
  // a range of consecutive cells is a view of the caller's arrays, any other range is gathered on the device; the few barcodes the tie
  // arbiter has to re-evaluate (near-tie flags, an open tie-order certificate) have their pieces of the pileup fetched when their range is written.
  const bool dev_pl = pl.memory == DMX_MEM_DEVICE;
  const dmx_pileup pl_dev = pl;                    // what the engines are given
  std::vector<int64_t> h_po, h_ro;
  if (dev_pl) {
    if (job->n_gpus > 1) return set_error(DMX_ERR_ARG, "dmx_demuxlet_run: a device-resident pileup lives on one GPU (n_gpus = %d)", job->n_gpus);
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return set_error(DMX_ERR_NOGPU, "dmx_demuxlet_run: no HIP device is visible (this library has no CPU fallback)");
    HIP_TRY(hipSetDevice(job->device % nd));
    h_po.resize((size_t)pl.n_cells + 1); h_ro.resize((size_t)pl.n_cells + 1);
    HIP_TRY(hipMemcpy(h_po.data(), pl.cell_pair_off, sizeof(int64_t) * ((size_t)pl.n_cells + 1), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_ro.data(), pl.cell_read_off, sizeof(int64_t) * ((size_t)pl.n_cells + 1), hipMemcpyDeviceToHost));
    if (h_po[0] != 0 || h_po[(size_t)pl.n_cells] != pl.n_pairs || h_ro[0] != 0 || h_ro[(size_t)pl.n_cells] != pl.n_reads)
      return set_error(DMX_ERR_ARG, "dmx_demuxlet_run: job->pileup's offset arrays do not span n_pairs / n_reads");
    for (int32_t c = 0; c < pl.n_cells; ++c)
      if (h_po[(size_t)c + 1] < h_po[(size_t)c] || h_ro[(size_t)c + 1] < h_ro[(size_t)c]) return set_error(DMX_ERR_ARG, "dmx_demuxlet_run: job->pileup's offsets are not monotone at cell %d", c);
    pl.cell_pair_off = h_po.data(); pl.cell_read_off = h_ro.data();      // the host logic below reads offsets only; the big arrays stay device pointers
  }
  if (job->n_samples < 1 || job->n_alpha < 1) return set_error(DMX_ERR_ARG, "dmx_demuxlet_run: n_samples %d, n_alpha %d", job->n_samples, job->n_alpha);
  for (int32_t j = 0; j < job->n_samples; ++j) if (!job->sample_ids[j]) return set_error(DMX_ERR_ARG, "dmx_demuxlet_run: sample_ids[%d] is null", j);
  tm.freeze_s = secs(t_begin, clk::now());
  const clk::time_point t_setup = clk::now();
  const int32_t B = pl.n_cells, V = job->n_samples, A = job->n_alpha;
  const size_t nAB = (size_t)V * V * A;
  const bool doublet_ok = V >= 2 && A >= 2;
  std::vector<const char*> bcs((size_t)B);
  std::vector<int32_t> nsnp((size_t)B);
  for (int32_t c = 0; c < B; ++c) {
    bcs[c] = job->store ? dmx_store_barcode(job->store, c) : job->barcodes[c];
    nsnp[c] = (int32_t)(pl.cell_pair_off[c + 1] - pl.cell_pair_off[c]);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_error(DMX_ERR_NOGPU, "dmx_demuxlet_run: no HIP device is visible (this library has no CPU fallback)");

  // ---- ranges: contiguous runs of the byte-wise sorted barcodes (= output order, cmd_cram_demuxlet.cpp:472,:576) with equal
  // work.  One engine per GPU; a range is what one engine holds at a time, sized so that its doublet grid stays inside a
  // byte budget (the grid, nb * V*V*A doubles, is the only thing that grows with the panel).  Ranges go through the engines
  // in waves; while the host arbitrates, formats and appends the rows of wave w, the GPUs already compute wave w + 1 — so a
  // job that is big enough is cut into at least four ranges per engine even when memory does not ask for it.
  const int ngpu = std::max(1, std::min(job->n_gpus > 0 ? job->n_gpus : 1, std::max(B, 1)));
  // How a job is cut is decided here and nowhere else: the three variables that override it (tests force many ranges, experiments time the
  // overlap) are read only behind the experiment fence, like the engines' own switches — a stray DMX_* variable cannot change a user's ranges
  const bool fence_open = [] { const char* x = getenv("DMX_EXPERIMENTS"); return x && x[0] == '1' && !x[1]; }();
  auto job_knob = [&](const char* name) -> const char* { return fence_open ? getenv(name) : nullptr; };
  size_t budget = (size_t)4 << 30;                                   // bytes of grid per range (host holds two waves of them)
  if (const char* env = job_knob("DMX_RANGE_BYTES")) budget = (size_t)std::max(1ll, atoll(env));   // tests: force many ranges
  {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipSetDevice(job->device % ndev));
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b / 6 < budget) budget = std::max<size_t>(free_b / 6, 1);   // two ranges per GPU in flight
  }
  const double per_pair = (double)(V + 1) + (doublet_ok ? (double)nAB + A : 0.0);
  double work_total = 0;
  for (int32_t c = 0; c < B; ++c) work_total += nsnp[c] * per_pair + 1.0;
  const double grid_total = doublet_ok ? (double)B * (double)nAB * 8.0 : 0.0;
  const int by_mem = (int)std::min<double>((double)std::max(B, 1), std::ceil(grid_total / (double)budget));
  int by_overlap = 1;                                                // ranges per engine wanted for host/GPU overlap
  if (const char* env = job_knob("DMX_RANGES_PER_GPU")) by_overlap = std::max(1, atoi(env));
  else {
    // worth it when an engine has more than ~0.15 s of kernels ahead of it (at ~6e11 evaluations/s; FAST evaluates the printed
    // entries only): the host then writes range r and stages r + 2 while the GPU computes r + 1
    const bool sym = job->mode == DMX_MODE_FAST && A == 2 && job->alpha[0] == 0.0 && job->alpha[1] == 0.5 && V <= 512;
    const double evals = (double)(V + 1) + (doublet_ok ? (sym ? (double)V + 0.5 * V * (V + 1) : (double)nAB) : 0.0);
    // A device-resident pileup has nothing to stage: what ranges buy there is only the writer thread's overlap (0.06-0.08 s at cfg3 size), and
    // they cost GPU time — a range of 2 500 one-barcode wavefronts fills 3 072 slots less well than one launch of 10 000, and two engines'
    // workgroups interleave so that both ranges finish together.  Measured at cfg3 size, FAST / STRICT: one range 0.383 / 1.29 s, two 0.407 /
    // 1.31, four 0.55 / 1.39 (profiles/r05_e2e_ranges.txt; chaining the ranges by events was worse still).  So such a job is cut only when
    // every range still makes several full rounds of wavefronts.
    const int min_cells = dev_pl ? 40 * 1024 : 8 * 1024;
    if (doublet_ok && (double)pl.n_pairs * evals / ngpu > 0.15 * 6e11 && B / ngpu >= min_cells) by_overlap = 4;
  }
  int R = std::max(ngpu * by_overlap, by_mem);
  R = ((R + ngpu - 1) / ngpu) * ngpu;                                 // whole waves
  R = std::max(1, std::min(R, std::max(B, 1)));
  const size_t cell_cap = doublet_ok ? std::max<size_t>(1, budget / (nAB * 8)) : (size_t)B + 1;   // a range never holds more cells than its grid budget
  std::vector<int32_t> order((size_t)B);
  std::iota(order.begin(), order.end(), 0);
  const bool sliced = R > 1;
  if (sliced) std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return std::strcmp(bcs[a], bcs[b]) < 0; });
  std::vector<int32_t> cut;
  cut.push_back(0);
  {
    double run = 0;
    int r = 1;
    for (int32_t i = 0; i < B; ++i) {
      run += nsnp[order[i]] * per_pair + 1.0;
      const bool by_work = r < R && run >= work_total * r / R;
      const bool by_cap = (size_t)(i + 1 - cut.back()) >= cell_cap;
      if ((by_work || by_cap) && i + 1 < B) { cut.push_back(i + 1); if (by_work) ++r; }
    }
    cut.push_back(B);
    if (B == 0) cut.assign({0, 0});
  }
  R = (int)cut.size() - 1;
  tm.n_ranges = R;

  struct Range {
    std::vector<int32_t> totl, pass, uniq, ns;
    std::vector<const char*> bc;
    std::vector<double> llks, llk0s, grid, l00, sing;
    std::vector<dmx_cell_summary> summ;
    std::vector<std::vector<double>> flagged_grid;
    std::vector<const double*> cell_grid;
    // device-resident pileups: the host pieces of the barcodes the tie arbiter may have to walk (tie_cell[k] = index here, -1 = not staged)
    std::vector<int32_t> tie_cell, t_snp; std::vector<int64_t> t_po, t_ro; std::vector<uint8_t> t_nrd, t_reads;
    // write_pair with the rows formatted on the device: the packed text (device memory, owned by the range until it is written) and its output cells
    dmx_pair_text* ptext = nullptr; std::vector<int32_t> out_cells;
    int32_t lo = 0, hi = 0;
    void release() { if (ptext) dmx_pair_text_free(ptext); *this = Range(); }
  };
  std::vector<Range> rg((size_t)R);
  struct RangeGuard { std::vector<Range>* r; ~RangeGuard() { for (Range& x : *r) if (x.ptext) { dmx_pair_text_free(x.ptext); x.ptext = nullptr; } } } range_guard{&rg};
  // `.pair` rows are formatted on the device (dmx_engine_format_pair) unless the fenced DMX_PAIR_ON_HOST=1 asks for the host formatter (tests compare the two)
  // or the job is beyond the device path's limits (pair_device_limit over ALL barcodes of the job, so every range decides alike): the host formatter then
  bool gpu_pair = job->write_pair && doublet_ok && !job_knob("DMX_PAIR_ON_HOST");
  if (gpu_pair) {
    size_t bc_max = 0, sm_max = 0, al_max = 0;
    bool prints = true;
    for (int32_t c = 0; c < B; ++c) bc_max = std::max(bc_max, std::strlen(bcs[(size_t)c]));
    for (int32_t j = 0; j < V; ++j) sm_max = std::max(sm_max, std::strlen(job->sample_ids[j]));
    for (int32_t a = 0; a < A; ++a) { std::string txt; prints = prints && pair_alpha_text(job->alpha[a], &txt); al_max = std::max(al_max, txt.size()); }
    if (!prints || pair_device_limit(V, A, bc_max, sm_max, al_max, nullptr)) gpu_pair = false;
  }
  double pair_format_ms = 0; int64_t pair_bytes = 0, pair_patches = 0, pair_host_cells = 0;
  // Engines: one per GPU and wave slot.  When the job takes several waves, every GPU gets TWO engines (own stream, own buffers)
  // that alternate between waves, so that the slicing + H2D of wave w + 2 overlaps the kernels of wave w + 1 (the copy engine
  // runs beside the compute units) while the host arbitrates and writes wave w.
  const int per_wave = std::min(ngpu, R);
  const int waves = (R + per_wave - 1) / per_wave;
  const int nset = (waves >= 2 && !job_knob("DMX_ONE_ENGINE_PER_GPU")) ? 2 : 1;
  std::vector<dmx_engine*> eng((size_t)per_wave * nset, nullptr);
  tm.n_engines = (int32_t)eng.size();
  struct Guard { std::vector<dmx_engine*>* e; ~Guard() { for (dmx_engine* x : *e) if (x) dmx_engine_destroy(x); } } guard{&eng};
  {
    auto make = [&](size_t i) -> int {
      dmx_engine_config cfg{};
      cfg.n_samples = V; cfg.n_alpha = A; cfg.alpha = job->alpha; cfg.doublet_prior = job->doublet_prior;
      cfg.device = (job->device + (int)(i % (size_t)per_wave)) % ndev; cfg.mode = job->mode;
      if (!job->arbiter) cfg.flags |= DMX_ENGINE_NO_CERTIFY;
      if (int rc = dmx_engine_create(&cfg, &eng[i])) return rc;
      return dmx_engine_set_genotypes(eng[i], job->g, pl.n_snps, DMX_MEM_HOST);
    };
    if (int rc = make(0)) return rc;              // the first one builds the host-side seed tables the others reuse
    std::vector<int> rcs(eng.size(), DMX_OK);
    std::vector<std::string> msgs(eng.size());
    std::vector<std::thread> th;
    for (size_t i = 1; i < eng.size(); ++i) th.emplace_back([&, i] { rcs[i] = make(i); if (rcs[i]) msgs[i] = dmx_last_error(); });
    for (std::thread& t : th) t.join();
    for (size_t i = 1; i < eng.size(); ++i) if (rcs[i]) return set_error(rcs[i], "%s", msgs[i].c_str());
  }
  tm.setup_s = secs(t_setup, clk::now());
  std::mutex tm_mu;
  const bool trace = getenv("DMX_E2E_TRACE") != nullptr;     // per-range timeline on stderr (seconds since the call began)
  auto mark = [&](const char* what, int r, clk::time_point t0) {
    if (trace) fprintf(stderr, "[dmx_demuxlet_run] %-6s range %d: %.4f -> %.4f s\n", what, r, secs(t_begin, t0), secs(t_begin, clk::now()));
  };
  double stage_s = 0, wait_s = 0, write_s = 0, kernel_ms = 0;
  int32_t n_fetched = 0;

  auto make_fin = [&](Range& x) {
    dmx_final_input fin{};
    fin.n_cells = x.hi - x.lo; fin.n_samples = V; fin.n_alpha = A; fin.alpha = job->alpha; fin.doublet_prior = job->doublet_prior;
    fin.min_total = job->min_total; fin.min_uniq = job->min_uniq; fin.min_snp = job->min_snp; fin.write_pair = job->write_pair;
    fin.sample_ids = job->sample_ids;
    if (sliced) { fin.barcodes = x.bc.data(); fin.rd_totl = x.totl.data(); fin.rd_pass = x.pass.data(); fin.rd_uniq = x.uniq.data(); fin.n_snp = x.ns.data(); }
    else { fin.barcodes = bcs.data(); fin.rd_totl = pl.rd_totl; fin.rd_pass = pl.rd_pass; fin.rd_uniq = pl.rd_uniq; fin.n_snp = nsnp.data(); }
    return fin;
  };
  auto eng_of = [&](int r) -> dmx_engine* { return eng[(size_t)(((r / per_wave) % nset) * per_wave + r % per_wave)]; };
  auto launch = [&](int r) -> int {              // stage range r on its engine and start its kernels (asynchronous)
    const clk::time_point t0 = clk::now();
    Range& x = rg[(size_t)r];
    x.lo = cut[(size_t)r]; x.hi = cut[(size_t)r + 1];
    const int32_t nb = x.hi - x.lo;
    if (sliced) {                                // cells order[lo..hi) become cells 0..nb-1 of the range: the small per-cell arrays
      const size_t nb1 = (size_t)std::max(nb, 1);                      // here, the CSR itself while it streams to the device
      x.totl.resize(nb1); x.pass.resize(nb1); x.uniq.resize(nb1); x.ns.resize(nb1); x.bc.resize(nb1);
      for (int32_t k = 0; k < nb; ++k) {
        const int32_t c = order[(size_t)x.lo + k];
        x.totl[(size_t)k] = pl.rd_totl[c]; x.pass[(size_t)k] = pl.rd_pass[c]; x.uniq[(size_t)k] = pl.rd_uniq[c];
        x.ns[(size_t)k] = nsnp[(size_t)c]; x.bc[(size_t)k] = bcs[(size_t)c];
      }
    }
    dmx_engine* e = eng_of(r);
    if (dev_pl) { if (int rc = dmx::engine_set_pileup_cells(e, &pl_dev, sliced ? order.data() + x.lo : nullptr, nb, h_po.data(), h_ro.data())) return rc; }
    else if (int rc = dmx::engine_set_pileup_cells(e, &pl, sliced ? order.data() + x.lo : nullptr, nb)) return rc;
    if (doublet_ok) { if (int rc = dmx_engine_run(e)) return rc; }
    else if (int rc = dmx_engine_run_singlet(e)) return rc;
    { std::lock_guard<std::mutex> lk(tm_mu); stage_s += secs(t0, clk::now()); }
    mark("launch", r, t0);
    return DMX_OK;
  };
  auto fetch = [&](int r) -> int {               // results of range r to the host (waits for its kernels)
    const clk::time_point t0 = clk::now();
    Range& x = rg[(size_t)r];
    const size_t nb = (size_t)(x.hi - x.lo), nb1 = std::max<size_t>(nb, 1);
    dmx_engine* e = eng_of(r);
    x.llks.resize(nb1 * (size_t)V); x.llk0s.resize(nb1);
    if (int rc = dmx_engine_get_singlet(e, x.llks.data(), x.llk0s.data())) return rc;
    int32_t fetched = 0;
    if (doublet_ok) {
      x.l00.resize(nb1 * (size_t)A);
      if (gpu_pair) {
        // .pair from the device: the records as below; the barcodes whose printed entries the arbiter may replace (dmx::cell_needs, a BEST-rule comparison
        // within 1e-7 — decided on the record AFTER resolve_tie_order, as the writers do) keep the host formatter and bring their grids
        x.sing.resize(nb1 * (size_t)V); x.summ.resize(nb1);
        if (int rc = dmx_engine_get_doublet(e, nullptr, x.l00.data(), x.summ.data())) return rc;
        if (int rc = dmx_engine_get_sing(e, x.sing.data())) return rc;
        x.cell_grid.assign(nb1, nullptr);
        const dmx_final_input fin = make_fin(x);
        x.out_cells = dmx::output_cells(&fin, true);
        const size_t n_out = x.out_cells.size();
        std::vector<uint8_t> host_rows(std::max<size_t>(n_out, 1), 0);
        std::vector<dmx_pair_override> ovr(std::max<size_t>(n_out, 1));
        std::vector<const char*> obc(std::max<size_t>(n_out, 1), nullptr);
        std::vector<int32_t> hostc;
        constexpr int32_t kNear = DMX_CELL_NEAR_DOUBLET | DMX_CELL_NEAR_SINGLET;
        for (size_t i = 0; i < n_out; ++i) {
          const size_t c = (size_t)x.out_cells[i];
          dmx_cell_summary sm = x.summ[c];
          if (sm.flags & DMX_CELL_ORDER_RESOLVABLE) (void)dmx::resolve_tie_order(&sm);
          const double* sg = x.sing.data() + c * (size_t)V;
          const bool rule = job->arbiter && sm.n_pairs > 0 &&
                            dmx::near_rule(sm.llk12, sm.llk1, sm.llk2, sg[std::max(sm.i_sing1, 0)], sg[std::max(sm.i_sing2, 0)], 1e-7);
          host_rows[i] = (dmx::cell_needs(sm, job->alpha, A, job->arbiter != 0) != 0 || rule) ? 1 : 0;
          ovr[i] = dmx_pair_override{-1, -1, -1, 0, 0.0, 0.0};
          if ((sm.flags & DMX_CELL_ORDER_CERTIFIED) && !(sm.flags & kNear) && sm.j_best >= 0 && sm.k_best >= 0)
            ovr[i] = dmx_pair_override{std::min(sm.j_best, sm.k_best), std::max(sm.j_best, sm.k_best), sm.n_best, 0, sm.llk_ab, sm.llk_ba};
          obc[i] = fin.barcodes[c];
          if (host_rows[i]) hostc.push_back((int32_t)c);
        }
        dmx_pair_request rq{};
        rq.n_out = (int32_t)n_out; rq.cells = x.out_cells.data(); rq.barcodes = obc.data(); rq.sample_ids = job->sample_ids;
        rq.host_rows = host_rows.data(); rq.ovr = ovr.data();
        if (int rc = dmx_engine_format_pair(e, &rq, &x.ptext)) return rc;
        dmx_pair_text_info pi{};
        (void)dmx_pair_text_get_info(x.ptext, &pi);
        for (size_t i = 0; i < n_out; ++i) if (pi.cell_flag[i] == 2) hostc.push_back(x.out_cells[i]);   // an unprintable entry: the host's printf prints it
        HIP_TRY(hipSetDevice(e->device));
        for (int32_t c : hostc) {
          x.flagged_grid.emplace_back(nAB);
          HIP_TRY(hipMemcpyAsync(x.flagged_grid.back().data(), e->d_grid + (size_t)c * nAB, sizeof(double) * nAB, hipMemcpyDeviceToHost, e->stream));
        }
        HIP_TRY(hipStreamSynchronize(e->stream));
        for (size_t f = 0; f < hostc.size(); ++f) x.cell_grid[(size_t)hostc[f]] = x.flagged_grid[f].data();
        fetched = (int32_t)hostc.size();
        { std::lock_guard<std::mutex> lk(tm_mu); pair_format_ms += pi.format_ms; pair_bytes += pi.n_bytes; pair_patches += pi.n_patches; pair_host_cells += (int64_t)hostc.size(); }
      } else if (job->write_pair) {              // .pair prints the grid: bring all of it (DMX_PAIR_ON_HOST: the host formatter)
        x.grid.resize(nb1 * nAB); x.summ.resize(nb1);
        if (int rc = dmx_engine_get_doublet(e, x.grid.data(), x.l00.data(), x.summ.data())) return rc;
      } else {                                   // otherwise the K3 records say everything, except for cells flagged as near-ties
        x.sing.resize(nb1 * (size_t)V); x.summ.resize(nb1);
        if (int rc = dmx_engine_get_doublet(e, nullptr, x.l00.data(), x.summ.data())) return rc;
        if (int rc = dmx_engine_get_sing(e, x.sing.data())) return rc;
        x.cell_grid.assign(nb1, nullptr);
        if (job->arbiter) {                       // (dmx::cell_needs: the one predicate the writers use too)
          for (size_t c = 0; c < nb; ++c) if (dmx::cell_needs(x.summ[c], job->alpha, A, true) & dmx::kNeedGrid) {
            x.flagged_grid.emplace_back(nAB);
            HIP_TRY(hipSetDevice(e->device));
            HIP_TRY(hipMemcpyAsync(x.flagged_grid.back().data(), e->d_grid + c * nAB, sizeof(double) * nAB, hipMemcpyDeviceToHost, e->stream));
            ++fetched;
          }
          HIP_TRY(hipStreamSynchronize(e->stream));
          size_t f = 0;
          for (size_t c = 0; c < nb; ++c) if (dmx::cell_needs(x.summ[c], job->alpha, A, true) & dmx::kNeedGrid) x.cell_grid[c] = x.flagged_grid[f++].data();
        }
      }
    }
    if (dev_pl && doublet_ok && job->arbiter) {
      // which barcodes can the writers' arbiter touch?  dmx::cell_needs says (a near-tie flag, a best doublet at alpha = 0.5 without a
      // (resolved) tie-order certificate, a BEST-rule comparison within 1e-7) — the predicate write_doublet_core itself checks before it
      // writes.  Their pairs and read bytes come to the host now.
      const size_t w = (size_t)pl.nrd_width;
      x.tie_cell.assign(nb1, -1);
      x.t_po.assign(1, 0); x.t_ro.assign(1, 0);
      std::vector<int32_t> need;
      for (size_t k = 0; k < nb; ++k) {
        dmx_cell_summary sm = x.summ[k];
        if (sm.n_pairs <= 0) continue;
        if (sm.flags & DMX_CELL_ORDER_RESOLVABLE) (void)dmx::resolve_tie_order(&sm);
        if (!(dmx::cell_needs(sm, job->alpha, A, true) & dmx::kNeedPileup)) continue;
        const int32_t c = sliced ? order[(size_t)x.lo + k] : (int32_t)k;
        x.tie_cell[k] = (int32_t)need.size();
        need.push_back(c);
        x.t_po.push_back(x.t_po.back() + (pl.cell_pair_off[c + 1] - pl.cell_pair_off[c]));
        x.t_ro.push_back(x.t_ro.back() + (pl.cell_read_off[c + 1] - pl.cell_read_off[c]));
      }
      x.t_nrd.resize((size_t)x.t_po.back() * w + 4); x.t_reads.resize((size_t)x.t_ro.back() + 4);
      if (pl.pair_snp) x.t_snp.resize((size_t)x.t_po.back() + 1);
      HIP_TRY(hipSetDevice(e->device));
      for (size_t i = 0; i < need.size(); ++i) {
        const int32_t c = need[i];
        const int64_t p0 = pl.cell_pair_off[c], np_ = pl.cell_pair_off[c + 1] - p0, r0 = pl.cell_read_off[c], nr_ = pl.cell_read_off[c + 1] - r0;
        if (np_ > 0) {
          if (pl.pair_snp) HIP_TRY(hipMemcpyAsync(x.t_snp.data() + x.t_po[i], pl.pair_snp + p0, sizeof(int32_t) * (size_t)np_, hipMemcpyDeviceToHost, e->stream));
          HIP_TRY(hipMemcpyAsync(x.t_nrd.data() + (size_t)x.t_po[i] * w, (const uint8_t*)pl.pair_nrd + (size_t)p0 * w, (size_t)np_ * w, hipMemcpyDeviceToHost, e->stream));
        }
        if (nr_ > 0) HIP_TRY(hipMemcpyAsync(x.t_reads.data() + x.t_ro[i], pl.reads + r0, (size_t)nr_, hipMemcpyDeviceToHost, e->stream));
      }
      HIP_TRY(hipStreamSynchronize(e->stream));
    }
    dmx_kernel_times kt{};
    (void)dmx_engine_last_kernel_times(e, &kt);
    { std::lock_guard<std::mutex> lk(tm_mu); wait_s += secs(t0, clk::now()); kernel_ms += kt.singlet_ms + kt.doublet_ms + kt.reduce_ms; n_fetched += fetched; }
    mark("fetch", r, t0);
    if (trace) fprintf(stderr, "[dmx_demuxlet_run]        range %d kernels: K1 %.1f ms, K2 %.1f ms, K3+K3b %.1f ms\n", r, kt.singlet_ms, kt.doublet_ms, kt.reduce_ms);
    return DMX_OK;
  };
  const std::string pre(job->out_prefix);
  // The .pair file of a range whose rows were formatted on the device: the packed text comes over in pieces through one pinned buffer and goes to
  // write(2) as it is; where the device left a POSTPRB field to the host (dmx_pair_patch: the denormal range, a digit next to a rounding boundary) the
  // field is computed here with the host libm — the expression of :780 / :792 on the three scalars the text itself was printed from (the K3 record,
  // or the certified grid's: dmx_pair_text_get_scalars) — and spliced in; barcodes left to the host
  // formatter (cell_flag != 0) have their rows (pair_rows, from write_doublet_core) inserted at their place.
  PinnedBuf pair_stage;
  constexpr int64_t kPairStage = (int64_t)32 << 20;
  auto stream_pair = [&](Range& x, const std::vector<std::string>& pair_rows, bool append) -> int {
    dmx_pair_text_info pi{};
    if (int rc = dmx_pair_text_get_info(x.ptext, &pi)) return rc;
    const dmx_pair_scalars* scal = nullptr;
    if (int rc = dmx_pair_text_get_scalars(x.ptext, &scal)) return rc;
    FILE* f = fopen((pre + ".pair").c_str(), append ? "a" : "w");
    if (!f) return set_error(DMX_ERR_IO, "Cannot create %s.single, %s.pair files", job->out_prefix, job->out_prefix);     // :535-536
    struct Closer { FILE* f; ~Closer() { if (f) fclose(f); } } closer{f};
    if (!append) fputs("BARCODE\tSM1.ID\tSM2.ID\tLLK12\tPOSTPRB\n", f);                                               // :570
    if (int rc = pair_stage.ensure((size_t)kPairStage)) return rc;
    char* buf = (char*)pair_stage.get();
    int64_t wbeg = 0, wend = 0;                  // the piece of the text the buffer holds
    bool ok = true;
    auto put = [&](int64_t a, int64_t b) -> int {     // text bytes [a, b)
      while (a < b) {
        if (a < wbeg || a >= wend) {
          wbeg = a; wend = std::min(pi.n_bytes, a + kPairStage);
          if (int rc = dmx_pair_text_read(x.ptext, wbeg, wend - wbeg, buf)) return rc;
        }
        const int64_t n = std::min(b, wend) - a;
        if (fwrite(buf + (a - wbeg), 1, (size_t)n, f) != (size_t)n) ok = false;
        a += n;
      }
      return DMX_OK;
    };
    int32_t ip = 0;
    std::string field;
    int64_t run_beg = 0;                         // consecutive device-formatted barcodes go out as one run
    for (int32_t oc = 0; oc < pi.n_out; ++oc) {
      const int64_t cb = pi.cell_off[oc], ce = pi.cell_off[oc + 1];
      if (pi.cell_flag[oc] != 0) {
        if (int rc = put(run_beg, cb)) return rc;
        const std::string& rows = pair_rows[(size_t)x.out_cells[(size_t)oc]];
        if (!rows.empty() && fwrite(rows.data(), 1, rows.size(), f) != rows.size()) ok = false;
        run_beg = ce;
        continue;
      }
      while (ip < pi.n_patches && pi.patches[ip].offset < ce) {
        const dmx_pair_patch& pp = pi.patches[ip++];
        if (int rc = put(run_beg, pp.offset)) return rc;
        run_beg = pp.offset;
        const dmx_pair_scalars& sm = scal[pp.out_cell];
        const double tot = sm.sum_single + sm.sum_double, prior = job->doublet_prior;
        const double p = pp.singlet ? std::exp(pp.value - sm.max_llk) * (1. - prior) / V / tot
                                    : std::exp(pp.value - sm.max_llk) * prior / V / (V - 1) / (A - 1) / tot;
        field.clear();
        dmx::put_general(field, p, 5);
        if (fwrite(field.data(), 1, field.size(), f) != field.size()) ok = false;
      }
    }
    if (int rc = put(run_beg, pi.n_bytes)) return rc;
    closer.f = nullptr;
    if (fclose(f) != 0 || !ok) return set_error(DMX_ERR_IO, "write failed (%s.pair)", job->out_prefix);
    return DMX_OK;
  };
  auto write = [&](int r) -> int {               // append range r's rows (rows of a range are sorted by the writers)
    const clk::time_point t0 = clk::now();
    Range& x = rg[(size_t)r];
    dmx_final_input fin = make_fin(x);
    fin.llks = x.llks.data(); fin.llk0s = x.llk0s.data();
    if (int rc = dmx::write_single_impl(&fin, (pre + ".single").c_str(), r > 0)) return rc;
    if (doublet_ok) {
      fin.llks00 = x.l00.data();
      dmx_pileup tie{};                          // device-resident pileups: the staged pieces of this range's arbiter barcodes
      if (job->arbiter && dev_pl) {
        tie.n_cells = (int32_t)x.t_po.size() - 1; tie.n_snps = pl.n_snps; tie.n_pairs = x.t_po.back(); tie.n_reads = x.t_ro.back();
        tie.cell_pair_off = x.t_po.data(); tie.cell_read_off = x.t_ro.data(); tie.pair_snp = pl.pair_snp ? x.t_snp.data() : nullptr;
        tie.pair_nrd = x.t_nrd.data(); tie.nrd_width = pl.nrd_width; tie.memory = DMX_MEM_HOST; tie.reads = x.t_reads.data();
        fin.tie_pileup = &tie; fin.tie_g = job->g;
      } else if (job->arbiter) { fin.tie_pileup = &pl; fin.tie_g = job->g; }
      dmx::DoubletSource src{};
      if (dev_pl) { if (job->arbiter) src.tie_cell = x.tie_cell.data(); }
      else if (sliced) src.tie_cell = order.data() + x.lo;
      std::vector<std::string> pair_rows;                     // device-formatted .pair: the rows of the barcodes left to the host formatter
      if (x.ptext) { pair_rows.resize((size_t)std::max(fin.n_cells, 1)); src.pair_rows = &pair_rows; }
      if (job->write_pair && !x.ptext) { fin.llksAB = x.grid.data(); src.grid_all = x.grid.data(); src.summary = x.summ.data(); }
      else { src.sing = x.sing.data(); src.summary = x.summ.data(); src.cell_grid = x.cell_grid.data(); }
      if (int rc = dmx::write_doublet_core(&fin, src, job->out_prefix, r > 0, "dmx_demuxlet_run")) return rc;
      if (x.ptext) if (int rc = stream_pair(x, pair_rows, r > 0)) return rc;
    }
    x.release();
    { std::lock_guard<std::mutex> lk(tm_mu); write_s += secs(t0, clk::now()); }
    mark("write", r, t0);
    return DMX_OK;
  };

  // the ranges of a wave belong to different engines: slice + stage (and later fetch) them on one host thread each, so that
  // eight GPUs are not fed one after the other (slicing a 2.8 GB shard out of the CSR is ~0.5 s of host memcpy)
  auto for_ranges = [&](int r0, int r1, const std::function<int(int)>& fn) -> int {
    if (r1 - r0 <= 1) { for (int r = r0; r < r1; ++r) if (int rc = fn(r)) return rc; return DMX_OK; }
    std::vector<int> rcs((size_t)(r1 - r0), DMX_OK);
    std::vector<std::string> msgs((size_t)(r1 - r0));
    std::vector<std::thread> th;
    for (int r = r0; r < r1; ++r)
      th.emplace_back([&, r] { const int rc = fn(r); rcs[(size_t)(r - r0)] = rc; if (rc) msgs[(size_t)(r - r0)] = dmx_last_error(); });
    for (std::thread& t : th) t.join();
    for (size_t i = 0; i < rcs.size(); ++i) if (rcs[i]) return set_error(rcs[i], "%s", msgs[i].c_str());   // the message is thread-local
    return DMX_OK;
  };
  auto wave_lo = [&](int w) { return std::min(R, w * per_wave); };
  // The rows of a fetched wave are arbitrated, formatted and appended by a writer thread, in range order, while this thread
  // stages and fetches the next waves; at most one wave waits for the writer when another is fetched (host memory: the results
  // of two waves, as the byte budget assumes).
  struct Writer {
    std::mutex mu; std::condition_variable cv; std::deque<int> q; bool closing = false; int pending = 0; int rc = DMX_OK; std::string msg; std::thread th;
    void close() { { std::lock_guard<std::mutex> lk(mu); closing = true; } cv.notify_all(); if (th.joinable()) th.join(); }
    ~Writer() { close(); }
  } wr;
  wr.th = std::thread([&] {
    for (;;) {
      int r;
      { std::unique_lock<std::mutex> lk(wr.mu); wr.cv.wait(lk, [&] { return !wr.q.empty() || wr.closing; }); if (wr.q.empty()) return; r = wr.q.front(); wr.q.pop_front(); }
      int rc = DMX_OK;
      { std::lock_guard<std::mutex> lk(wr.mu); rc = wr.rc; }
      if (rc == DMX_OK) { rc = write(r); if (rc) { std::lock_guard<std::mutex> lk(wr.mu); wr.rc = rc; wr.msg = dmx_last_error(); } }
      else rg[(size_t)r].release();
      { std::lock_guard<std::mutex> lk(wr.mu); --wr.pending; }
      wr.cv.notify_all();
    }
  });
  for (int w = 0; w < std::min(waves, nset); ++w) if (int rc = for_ranges(wave_lo(w), wave_lo(w + 1), launch)) return rc;
  for (int w = 0; w < waves; ++w) {
    { std::unique_lock<std::mutex> lk(wr.mu); wr.cv.wait(lk, [&] { return wr.pending <= per_wave; }); if (wr.rc) break; }
    if (int rc = for_ranges(wave_lo(w), wave_lo(w + 1), fetch)) return rc;
    { std::lock_guard<std::mutex> lk(wr.mu); for (int r = wave_lo(w); r < wave_lo(w + 1); ++r) { wr.q.push_back(r); ++wr.pending; } }
    wr.cv.notify_all();
    if (w + nset < waves) if (int rc = for_ranges(wave_lo(w + nset), wave_lo(w + nset + 1), launch)) return rc;   // the freed engines stage wave w + nset
  }
  wr.close();
  if (wr.rc) return set_error(wr.rc, "%s", wr.msg.c_str());
  tm.stage_s = stage_s; tm.wait_s = wait_s; tm.write_s = write_s; tm.kernel_ms = kernel_ms; tm.n_cells_grid_fetched = n_fetched;
  for (int32_t c = 0; c < B; ++c)                  // the droplets the reference counts at :480-524
    if (pl.rd_totl[c] >= job->min_total && pl.rd_uniq[c] >= job->min_uniq && nsnp[(size_t)c] >= job->min_snp) ++tm.n_cells_single;
  tm.total_s = secs(t_begin, clk::now());
  if (job->timing) *job->timing = tm;
  if (getenv("DMX_E2E_TIMING"))
    fprintf(stderr, "{\"dmx_demuxlet_run\": {\"freeze_s\": %.4f, \"setup_s\": %.4f, \"stage_s\": %.4f, \"wait_s\": %.4f, \"write_s\": %.4f, \"total_s\": %.4f, "
                    "\"kernel_ms\": %.3f, \"ranges\": %d, \"engines\": %d, \"cells_grid_fetched\": %d, \"pair_on_device\": %d, \"pair_format_ms\": %.3f, "
                    "\"pair_bytes\": %lld, \"pair_patches\": %lld, \"pair_host_cells\": %lld}}\n",
            tm.freeze_s, tm.setup_s, tm.stage_s, tm.wait_s, tm.write_s, tm.total_s, tm.kernel_ms, tm.n_ranges, tm.n_engines, tm.n_cells_grid_fetched,
            gpu_pair ? 1 : 0, pair_format_ms, (long long)pair_bytes, (long long)pair_patches, (long long)pair_host_cells);
  if (!doublet_ok) return set_error(DMX_ERR_ARG, "dmx_demuxlet_run: the doublet stage needs >= 2 samples and >= 2 alphas (got %d, %d)", V, A);
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Empirical-Bayes priors from the doublet grid.  prior_prepare checks the request, finds the grid (the engine's,
// the caller's device array, or a device copy of the caller's host array), stages the mask and sizes the buffers; prior_upload puts
// pi | d on the device and builds the log tables; prior_pass is one k_prior_estep + fold with V + 3 doubles copied back.
#include "dmx_prior.hpp"

namespace {

struct PriorPlan {
  int32_t B = 0, V = 0, A = 0, W = 4;
  size_t lds = 0;
  const double* grid = nullptr;
  const uint8_t* mask = nullptr;
};

int prior_prepare(dmx_engine* e, const char* fn, const dmx_prior_request* rq, bool for_call, PriorPlan* pl) {
  const int32_t V = e->V, A = e->A, B = rq->n_cells;
  if (rq->n_samples != V || rq->n_alpha != A)
    return set_error(DMX_ERR_ARG, "%s: n_samples %d, n_alpha %d; the engine has %d, %d", fn, rq->n_samples, rq->n_alpha, V, A);
  if (V < 2 || A < 2) return set_error(DMX_ERR_ARG, "%s: needs >= 2 samples and >= 2 alphas (got %d, %d)", fn, V, A);
  if ((int64_t)V * A > dmx_prior::kPriMaxVA) return set_error(DMX_ERR_ARG, "%s: n_samples x n_alpha = %lld, at most %d", fn, (long long)V * A, dmx_prior::kPriMaxVA);
  if ((int64_t)V * V * A >= ((int64_t)1 << 31)) return set_error(DMX_ERR_ARG, "%s: a grid of %d x %d x %d entries per barcode", fn, V, V, A);
  if (!rq->grid) {
    if (!e->have_grid) return set_error(DMX_ERR_STATE, "%s: no doublet grid (dmx_engine_run_doublet first, or pass a grid)", fn);
    if (B != e->pv.B) return set_error(DMX_ERR_ARG, "%s: n_cells %d, the staged pileup has %d", fn, B, e->pv.B);
  } else {
    if (B < 0) return set_error(DMX_ERR_ARG, "%s: n_cells %d", fn, B);
    if (rq->grid_memory != DMX_MEM_HOST && rq->grid_memory != DMX_MEM_DEVICE) return set_error(DMX_ERR_ARG, "%s: grid_memory %d", fn, rq->grid_memory);
  }
  if (B < 1) return set_error(DMX_ERR_ARG, "%s: no barcode (B_in == 0)", fn);
  HIP_TRY(hipSetDevice(e->device));
  const size_t sv = (size_t)V, sb = (size_t)B, gbytes = sizeof(double) * sb * sv * sv * (size_t)A;
  const size_t n_chunks = (sb + dmx_prior::kPriChunk - 1) / dmx_prior::kPriChunk;
  const size_t rows_b = sizeof(double) * sb * (sv + 3), part_b = sizeof(double) * n_chunks * (sv + 3), call_b = sizeof(dmx_prior_call) * sb;
  size_t free_b = 0, total_b = 0, need = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  auto want = [&](size_t bytes, size_t cap) { if (bytes > cap) need += bytes + bytes / 16; };
  if (rq->grid && rq->grid_memory == DMX_MEM_HOST) want(gbytes, e->d_prgrid.cap());
  if (for_call) want(call_b, e->d_prcall.cap()); else { want(rows_b, e->d_prrows.cap()); want(part_b, e->d_prpart.cap()); }
  want(sb, e->d_prmask.cap());
  if (!for_call) { want(sb, e->d_prflag.cap()); want(sizeof(int32_t) * sb, e->d_pridx.cap()); }
  if (need > free_b) return set_error(DMX_ERR_NOMEM, "%s: %d barcodes x %d samples need %zu more device bytes, %zu are free", fn, B, V, need, free_b);
  if (rq->grid && rq->grid_memory == DMX_MEM_HOST) {
    if (int rc = e->d_prgrid.ensure(gbytes)) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_prgrid, rq->grid, gbytes, hipMemcpyHostToDevice, e->stream));
    pl->grid = e->d_prgrid;
  } else {
    pl->grid = rq->grid ? rq->grid : (const double*)e->d_grid;
  }
  if (int rc = e->d_prmask.ensure(sb)) return rc;
  if (int rc = e->d_prnin.ensure(sizeof(int32_t))) return rc;
  if (int rc = e->d_prst.ensure(sizeof(double) * (sv + 1))) return rc;
  if (int rc = e->d_prtab.ensure(sizeof(double) * (3 * sv + 1))) return rc;
  if (int rc = e->d_prout.ensure(sizeof(double) * (2 * sv + 5))) return rc;
  if (for_call) {
    if (int rc = e->d_prcall.ensure(call_b)) return rc;
  } else {
    if (int rc = e->d_prrows.ensure(rows_b)) return rc;
    if (int rc = e->d_prpart.ensure(part_b)) return rc;
    if (int rc = e->d_prflag.ensure(sb)) return rc;
    if (int rc = e->d_pridx.ensure(sizeof(int32_t) * sb)) return rc;
  }
  if (rq->mask) {
    HIP_TRY(hipMemcpyAsync(e->d_prmask, rq->mask, sb, hipMemcpyHostToDevice, e->stream));
    pl->mask = e->d_prmask;
  } else if (!rq->grid) {
    hipLaunchKernelGGL(dmx_prior::k_prior_mask, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, e->stream, (const dmx_cell_summary*)e->d_sum, B,
                       e->d_prmask.get());
    HIP_TRY(hipGetLastError());
    pl->mask = e->d_prmask;
  } else {
    pl->mask = nullptr;
  }
  HIP_TRY(hipStreamSynchronize(e->stream));         // (the caller's host grid and mask may go away on return)
  // wavefronts per workgroup: the widest of 4, 2, 1 whose shared table, slots, rows and singlets fit 64 KiB (a barcode's bits do not depend on it)
  const size_t va = sv * (size_t)A;
  int32_t W = 4;
  while (W > 1 && sizeof(double) * (va + (size_t)W * (va + 2 * sv)) > 64 * 1024) W >>= 1;
  pl->B = B; pl->V = V; pl->A = A; pl->W = W;
  pl->lds = sizeof(double) * (va + (size_t)W * (va + 2 * sv));
  if (!e->have_pr_info) std::memset(&e->pr_info, 0, sizeof e->pr_info);
  e->pr_info.bytes_per_iter = (int64_t)gbytes; e->pr_info.n_cells = B; e->pr_info.n_samples = V; e->pr_info.n_alpha = A;
  e->pr_info.waves_per_block = W;
  e->have_pr_info = true;
  return DMX_OK;
}

// pi (any positive scale; NULL = uniform) and d: checked before a call touches any buffer, so that a refused call leaves the earlier results
int prior_check_params(const char* fn, int32_t V, const double* pi, double d) {
  if (!(d >= 0.0 && d <= 1.0)) return set_error(DMX_ERR_ARG, "%s: d = %g is not in [0, 1]", fn, d);
  double s = 0.0;
  for (int32_t j = 0; j < V; ++j) {
    const double x = pi ? pi[j] : 1.0;
    if (!(x >= 0.0 && x < INFINITY)) return set_error(DMX_ERR_ARG, "%s: pi[%d] = %g is negative or not finite", fn, j, x);
    s += x;
  }
  if (!(s > 0.0 && s < INFINITY)) return set_error(DMX_ERR_ARG, "%s: pi sums to %g", fn, s);
  return DMX_OK;
}

// pi / sum(pi) | d uploaded (the sum in ascending j), the tables built
int prior_upload(dmx_engine* e, const PriorPlan& pl, const double* pi, double d) {
  const int32_t V = pl.V;
  std::vector<double> st((size_t)V + 1);
  double s = 0.0;
  for (int32_t j = 0; j < V; ++j) s += pi ? pi[j] : 1.0;
  for (int32_t j = 0; j < V; ++j) st[(size_t)j] = (pi ? pi[j] : 1.0) / s;
  st[(size_t)V] = d;
  HIP_TRY(hipMemcpyAsync(e->d_prst, st.data(), sizeof(double) * st.size(), hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(dmx_prior::k_prior_tables, dim3(1), dim3(256), 0, e->stream, (const double*)e->d_prst, V, pl.A, e->d_prtab.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));         // (st goes away on return)
  return DMX_OK;
}

template <bool CALL>
int prior_launch_estep(dmx_engine* e, const PriorPlan& pl) {
  auto kern = &dmx_prior::k_prior_estep<CALL>;
  if (pl.lds > 30 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)((pl.B + pl.W - 1) / pl.W)), dim3(64 * pl.W), pl.lds, e->stream, pl.grid, pl.mask, pl.B, pl.V, pl.A,
                     (const double*)e->d_prtab, e->d_prrows.get(), e->d_prflag.get(), e->d_prcall.get());
  HIP_TRY(hipGetLastError());
  return DMX_OK;
}

// out[V + 3] = N | hom | het | LL at the device's (pi, d); full != NULL: all 2 V + 5 doubles (then pi' | d' | B_in)
int prior_pass(dmx_engine* e, const PriorPlan& pl, bool apply, bool fix_pi, bool fix_d, double* out, double* full) {
  const int32_t V = pl.V;
  if (int rc = e->prev[0].record_start(e->stream)) return rc;
  if (int rc = prior_launch_estep<false>(e, pl)) return rc;
  if (int rc = e->prev[0].record_stop(e->stream)) return rc;
  if (int rc = e->prev[1].record_start(e->stream)) return rc;
  const int32_t n_chunks = (pl.B + dmx_prior::kPriChunk - 1) / dmx_prior::kPriChunk;
  hipLaunchKernelGGL(dmx_prior::k_prior_rank, dim3(1), dim3(1024), 0, e->stream, (const uint8_t*)e->d_prflag, pl.B, e->d_pridx.get(), e->d_prnin.get());
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(dmx_prior::k_prior_fold_chunk, dim3((unsigned)n_chunks, (unsigned)((V + 3 + 63) / 64)), dim3(256), 0, e->stream, (const double*)e->d_prrows,
                     (const int32_t*)e->d_pridx, (const int32_t*)e->d_prnin, V, e->d_prpart.get());
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(dmx_prior::k_prior_fold, dim3(1), dim3(256), 0, e->stream, (const double*)e->d_prpart, (const int32_t*)e->d_prnin, V, pl.A,
                     apply ? 1 : 0, fix_pi ? 1 : 0, fix_d ? 1 : 0, e->d_prst.get(), e->d_prout.get(), e->d_prtab.get());
  HIP_TRY(hipGetLastError());
  if (int rc = e->prev[1].record_stop(e->stream)) return rc;
  if (out) HIP_TRY(hipMemcpyAsync(out, e->d_prout, sizeof(double) * ((size_t)V + 3), hipMemcpyDeviceToHost, e->stream));
  if (full) HIP_TRY(hipMemcpyAsync(full, e->d_prout, sizeof(double) * (2 * (size_t)V + 5), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  float ms0 = 0.f, ms1 = 0.f;
  if (int rc = e->prev[0].elapsed_ms(&ms0)) return rc;
  if (int rc = e->prev[1].elapsed_ms(&ms1)) return rc;
  e->pr_info.estep_ms = ms0; e->pr_info.fold_ms = ms1;
  return DMX_OK;
}

}  // namespace

extern "C" int dmx_engine_prior_step(dmx_engine* e, const dmx_prior_request* rq, const double* pi, double d) {
  const char* fn = "dmx_engine_prior_step";
  if (!e || !rq || !pi) return set_error(DMX_ERR_ARG, "%s: null argument", fn);
  PriorPlan pl;
  if (int rc = prior_check_params(fn, e->V, pi, d)) return rc;
  if (int rc = prior_prepare(e, fn, rq, false, &pl)) return rc;   // (a call refused up to here leaves the last step's results readable)
  e->have_pr_step = false;
  if (int rc = prior_upload(e, pl, pi, d)) return rc;
  e->pr_step_out.assign(2 * (size_t)pl.V + 5, 0.0);
  if (int rc = prior_pass(e, pl, false, false, false, nullptr, e->pr_step_out.data())) return rc;
  if (e->pr_step_out[2 * (size_t)pl.V + 4] < 1.0) return set_error(DMX_ERR_ARG, "%s: no barcode is included (B_in == 0)", fn);
  e->pr_B = pl.B; e->pr_V = pl.V;
  e->have_pr_step = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_prior_step(dmx_engine* e, double* N, double* hom, double* het, double* ll, int32_t* b_in, double* pi_next,
                                         double* d_next, double* rows, uint8_t* flags) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_prior_step: null engine");
  if (!e->have_pr_step) return set_error(DMX_ERR_STATE, "dmx_engine_get_prior_step: no step yet (dmx_engine_prior_step first)");
  const size_t V = (size_t)e->pr_V, B = (size_t)e->pr_B;
  const double* o = e->pr_step_out.data();
  if (N) std::memcpy(N, o, sizeof(double) * V);
  if (hom) *hom = o[V];
  if (het) *het = o[V + 1];
  if (ll) *ll = o[V + 2];
  if (pi_next) std::memcpy(pi_next, o + V + 3, sizeof(double) * V);
  if (d_next) *d_next = o[2 * V + 3];
  if (b_in) *b_in = (int32_t)o[2 * V + 4];
  HIP_TRY(hipSetDevice(e->device));
  if (rows) HIP_TRY(hipMemcpyAsync(rows, e->d_prrows, sizeof(double) * B * (V + 3), hipMemcpyDeviceToHost, e->stream));
  if (flags) HIP_TRY(hipMemcpyAsync(flags, e->d_prflag, B, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return DMX_OK;
}

extern "C" int dmx_engine_prior_fit(dmx_engine* e, const dmx_prior_request* rq) {
  const char* fn = "dmx_engine_prior_fit";
  if (!e || !rq) return set_error(DMX_ERR_ARG, "%s: null argument", fn);
  if (rq->max_iter < 1) return set_error(DMX_ERR_ARG, "%s: max_iter %d", fn, rq->max_iter);
  PriorPlan pl;
  if (int rc = prior_check_params(fn, e->V, rq->pi0, rq->d0)) return rc;
  if (int rc = prior_prepare(e, fn, rq, false, &pl)) return rc;
  e->have_pr_fit = false; e->have_pr_step = false;  // (the fit's passes overwrite the step's rows and flags)
  if (int rc = prior_upload(e, pl, rq->pi0, rq->d0)) return rc;
  const size_t V = (size_t)pl.V;
  std::vector<double> out(V + 3), full(2 * V + 5);
  e->pr_fit_ll.clear(); e->pr_fit_d.clear();
  double d_cur = rq->d0, fit_ms = 0.0, b_in = 0.0;
  int32_t conv = 0;
  for (int32_t it = 0; it < rq->max_iter; ++it) {
    // the first iteration also reads B_in and every iteration d' (the trace's next entry): V + 3 doubles decide the stop
    if (int rc = prior_pass(e, pl, true, rq->fix_pi != 0, rq->fix_d != 0, out.data(), it == 0 ? full.data() : nullptr)) return rc;
    fit_ms += e->pr_info.estep_ms + e->pr_info.fold_ms;
    if (it == 0) {
      b_in = full[2 * V + 4];
      if (b_in < 1.0) return set_error(DMX_ERR_ARG, "%s: no barcode is included (B_in == 0)", fn);
    }
    e->pr_fit_ll.push_back(out[V + 2]); e->pr_fit_d.push_back(d_cur);
    if (!rq->fix_d) d_cur = std::fmin((out[V] + out[V + 1]) / b_in, 1.0);     // (k_prior_fold's own expression)
    if (it > 0 && rq->tol > 0.0 && e->pr_fit_ll[(size_t)it] - e->pr_fit_ll[(size_t)it - 1] < rq->tol * b_in) { conv = 1; break; }
  }
  e->pr_fit_out.assign(2 * V + 5, 0.0);
  if (int rc = prior_pass(e, pl, false, true, true, nullptr, e->pr_fit_out.data())) return rc;   // the final evaluation: pi' = pi, d' = d
  e->pr_fit_pi.assign(e->pr_fit_out.begin() + (ptrdiff_t)(V + 3), e->pr_fit_out.begin() + (ptrdiff_t)(2 * V + 3));
  e->pr_fit_dd = e->pr_fit_out[2 * V + 3];
  e->pr_fit_iter = (int32_t)e->pr_fit_ll.size(); e->pr_fit_conv = conv;
  e->pr_info.n_iter = e->pr_fit_iter; e->pr_info.fit_ms = fit_ms;
  e->pr_B = pl.B; e->pr_V = pl.V;
  e->have_pr_fit = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_prior_fit(dmx_engine* e, double* pi, double* d, double* ll, int32_t* n_iter, int32_t* converged, int32_t* b_in,
                                        double* N, double* hom, double* het, double* ll_trace, double* d_trace, int32_t trace_cap) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_prior_fit: null engine");
  if (!e->have_pr_fit) return set_error(DMX_ERR_STATE, "dmx_engine_get_prior_fit: no fit yet (dmx_engine_prior_fit first)");
  const size_t V = (size_t)e->pr_V;
  const double* o = e->pr_fit_out.data();
  if (pi) std::memcpy(pi, e->pr_fit_pi.data(), sizeof(double) * V);
  if (d) *d = e->pr_fit_dd;
  if (ll) *ll = o[V + 2];
  if (n_iter) *n_iter = e->pr_fit_iter;
  if (converged) *converged = e->pr_fit_conv;
  if (b_in) *b_in = (int32_t)o[2 * V + 4];
  if (N) std::memcpy(N, o, sizeof(double) * V);
  if (hom) *hom = o[V];
  if (het) *het = o[V + 1];
  const size_t n = (size_t)std::max(0, std::min(trace_cap, e->pr_fit_iter));
  if (ll_trace) std::memcpy(ll_trace, e->pr_fit_ll.data(), sizeof(double) * n);
  if (d_trace) std::memcpy(d_trace, e->pr_fit_d.data(), sizeof(double) * n);
  return DMX_OK;
}

extern "C" int dmx_engine_prior_call(dmx_engine* e, const dmx_prior_request* rq, const double* pi, double d) {
  const char* fn = "dmx_engine_prior_call";
  if (!e || !rq || !pi) return set_error(DMX_ERR_ARG, "%s: null argument", fn);
  PriorPlan pl;
  if (int rc = prior_check_params(fn, e->V, pi, d)) return rc;
  if (int rc = prior_prepare(e, fn, rq, true, &pl)) return rc;   // (touches the records, never a step's rows or flags: a record carries its own flag)
  e->have_pr_call = false;
  if (int rc = prior_upload(e, pl, pi, d)) return rc;
  if (int rc = e->prev[2].record_start(e->stream)) return rc;
  if (int rc = prior_launch_estep<true>(e, pl)) return rc;
  if (int rc = e->prev[2].record_stop(e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  float ms = 0.f;
  if (int rc = e->prev[2].elapsed_ms(&ms)) return rc;
  e->pr_info.call_ms = ms;
  e->pr_call_B = pl.B;
  e->have_pr_call = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_prior_calls(dmx_engine* e, dmx_prior_call* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_get_prior_calls: null argument");
  if (!e->have_pr_call) return set_error(DMX_ERR_STATE, "dmx_engine_get_prior_calls: no records yet (dmx_engine_prior_call first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(out, e->d_prcall, sizeof(dmx_prior_call) * (size_t)e->pr_call_B, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return DMX_OK;
}

extern "C" int dmx_engine_prior_info(dmx_engine* e, dmx_prior_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_prior_info: null argument");
  if (!e->have_pr_info) return set_error(DMX_ERR_STATE, "dmx_engine_prior_info: no prior pass yet (dmx_engine_prior_step, _fit or _call first)");
  *out = e->pr_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Goodness of fit: the arguments are checked on the host (hyp, alpha, rho and a are small), the used barcodes'
// ids are listed singlets first, then one launch of k_fit<false, MM> over the singlets and one of k_fit<true, MM> over the doublets, MM
// the smallest of 1 / 2 / 4 / 8 that holds max_reads.  Every buffer is the call's own.
namespace {

template <bool DBL>
void launch_fit(dmx_engine* e, int32_t MMsel, const int32_t* idx, int32_t n_idx, int32_t M) {
  if (n_idx <= 0) return;
  const dim3 grid((unsigned)((n_idx + kFitWaves - 1) / kFitWaves)), block(64 * kFitWaves);
  const double* par = e->d_fpar;
  const int32_t B = e->pv.B;
#define DMX_FIT_LAUNCH(MMV)                                                                                                              \
  hipLaunchKernelGGL((k_fit<DBL, MMV>), grid, block, 0, e->stream, e->pv, e->nrd_width, (const double*)e->d_lut, e->d_g, e->V, idx, n_idx, \
                     (const int32_t*)e->d_fhyp, par, par + B, (const double*)e->d_famb, M, B, e->d_fout.get(), e->d_fcnt.get())
  if (MMsel == 1) DMX_FIT_LAUNCH(1);
  else if (MMsel == 2) DMX_FIT_LAUNCH(2);
  else if (MMsel == 4) DMX_FIT_LAUNCH(4);
  else DMX_FIT_LAUNCH(8);
#undef DMX_FIT_LAUNCH
}

}  // namespace

extern "C" int dmx_engine_fit(dmx_engine* e, const dmx_fit_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_fit: null argument");
  const char* fn = "dmx_engine_fit";
  if (int rc = require_staged(e, fn)) return rc;
  const int32_t B = e->pv.B, V = e->V, S = e->S, M = rq->max_reads;
  if (int rc = require_sizes(e, fn, rq->n_cells, rq->n_snps)) return rc;
  if (M < 1 || M > kFitMaxReads) return set_error(DMX_ERR_ARG, "dmx_engine_fit: max_reads %d is not in [1, %d]", M, kFitMaxReads);
  HypPlan pl{fn, B, V, S, rq->hyp, rq->hyp_memory, rq->alpha, rq->rho, rq->ambient};
  if (int rc = pl.check_args()) return rc;
  if (int rc = pl.check_ranges()) return rc;
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = pl.fetch(e)) return rc;
  if (int rc = pl.list()) return rc;
  const std::vector<int32_t>& idx = pl.idx;
  const int32_t n_sng = pl.n_sng, n_used = pl.n_used(), n_dbl = pl.n_dbl();
  const size_t out_b = sizeof(double) * 3 * (size_t)B, cnt_b = sizeof(int32_t) * 4 * (size_t)B, par_b = sizeof(double) * 2 * (size_t)B;
  const size_t need = out_b + cnt_b + par_b + sizeof(int32_t) * 3 * (size_t)B + sizeof(double) * (size_t)S;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (out_b > e->d_fout.cap() && need + need / 16 > free_b)
    return set_error(DMX_ERR_NOMEM, "dmx_engine_fit: the results of %d barcodes need %zu bytes, %zu are free", B, need, free_b);
  if (int rc = e->d_fout.ensure(out_b)) return rc;
  if (int rc = e->d_fcnt.ensure(cnt_b)) return rc;
  if (int rc = e->d_fpar.ensure(par_b)) return rc;
  if (int rc = e->d_fhyp.ensure(sizeof(int32_t) * 2 * (size_t)B)) return rc;
  if (int rc = e->d_fidx.ensure(sizeof(int32_t) * (size_t)B)) return rc;
  if (int rc = e->d_famb.ensure(sizeof(double) * (size_t)S)) return rc;
  e->have_fit = false;
  if (int rc = pl.upload(e, e->d_fhyp, e->d_fpar)) return rc;
  if (B > 0) {
    HIP_TRY(hipMemsetAsync(e->d_fout, 0, out_b, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_fcnt, 0, cnt_b, e->stream));
  }
  if (n_used > 0) HIP_TRY(hipMemcpyAsync(e->d_fidx, idx.data(), sizeof(int32_t) * (size_t)n_used, hipMemcpyHostToDevice, e->stream));
  if (int rc = stage_soup(e, rq->ambient, S, e->d_famb)) return rc;
  const int32_t MMsel = M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : 8;
  if (int rc = e->fev.record_start(e->stream)) return rc;
  launch_fit<false>(e, MMsel, e->d_fidx, n_sng, M);
  HIP_TRY(hipGetLastError());
  launch_fit<true>(e, MMsel, e->d_fidx + n_sng, n_dbl, M);
  HIP_TRY(hipGetLastError());
  if (int rc = e->fev.record_stop(e->stream)) return rc;
  std::vector<int32_t> tz((size_t)B * 2);
  if (B > 0) HIP_TRY(hipMemcpyAsync(tz.data(), e->d_fcnt + 2 * (size_t)B, sizeof(int32_t) * 2 * (size_t)B, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));        // the caller's inputs may go away after return
  float ms = 0.f;
  if (int rc = e->fev.elapsed_ms(&ms)) return rc;
  dmx_fit_info& inf = e->fit_info;
  std::memset(&inf, 0, sizeof inf);
  inf.kernel_ms = ms; inf.bytes = (int64_t)need; inf.n_cells = B; inf.n_used = n_used; inf.n_singlet = n_sng; inf.n_doublet = n_dbl;
  inf.max_reads = M;
  for (int32_t b = 0; b < B; ++b) { inf.n_trunc += tz[(size_t)b]; inf.n_zero += tz[(size_t)B + b]; }
  e->fit_B = B; e->have_fit = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_fit(dmx_engine* e, double* obs, double* mean, double* var, int32_t* n_snp, int32_t* n_read, int32_t* n_trunc,
                                  int32_t* n_zero) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_fit: null engine");
  if (!e->have_fit) return set_error(DMX_ERR_STATE, "dmx_engine_get_fit: no result on the staged pileup (dmx_engine_fit first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t B = (size_t)e->fit_B;
  if (!B) return DMX_OK;
  double* const dp[3] = {obs, mean, var};
  int32_t* const ip[4] = {n_snp, n_read, n_trunc, n_zero};
  for (int k = 0; k < 3; ++k)
    if (dp[k]) HIP_TRY(hipMemcpy(dp[k], e->d_fout + k * B, sizeof(double) * B, hipMemcpyDeviceToHost));
  for (int k = 0; k < 4; ++k)
    if (ip[k]) HIP_TRY(hipMemcpy(ip[k], e->d_fcnt + k * B, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_fit_info(dmx_engine* e, dmx_fit_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_fit_info: null argument");
  if (!e->have_fit) return set_error(DMX_ERR_STATE, "dmx_engine_fit_info: no result on the staged pileup (dmx_engine_fit first)");
  *out = e->fit_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Site audit: dmx_engine_fit's checks and lists, then the refinement's scheme — the slab table of the staged
// pileup (shared with the refinement: the same kernel at the same shift), per wave of chunks one launch of k_site_partial<false, MM>
// over the wave's singlet chunks, one of k_site_partial<true, MM> over its doublet chunks, and k_site_fold.
namespace {

template <bool DBL>
void launch_site_partial(dmx_engine* e, int32_t MMsel, int32_t nblk, const int32_t* d_mem, const int32_t* d_beg, int32_t c0, int32_t nc, int32_t row0,
                         int32_t M) {
  if (nc <= 0) return;
  const dim3 grid((unsigned)nblk, (unsigned)nc), block(64);
  const double* par = e->d_spar;
  const int32_t B = e->pv.B;
#define DMX_SITE_LAUNCH(MMV)                                                                                                                \
  hipLaunchKernelGGL((k_site_partial<DBL, MMV>), grid, block, 0, e->stream, e->pv, e->nrd_width, (const double*)e->d_lut, e->d_g, e->V,       \
                     (const int64_t*)e->d_rblk, nblk, d_mem, d_beg, c0, row0, (const int32_t*)e->d_shyp, par, par + B, (const double*)e->d_samb, \
                     M, e->d_spart.get())
  if (MMsel == 1) DMX_SITE_LAUNCH(1);
  else if (MMsel == 2) DMX_SITE_LAUNCH(2);
  else if (MMsel == 4) DMX_SITE_LAUNCH(4);
  else DMX_SITE_LAUNCH(8);
#undef DMX_SITE_LAUNCH
}

}  // namespace

extern "C" int dmx_engine_site_fit(dmx_engine* e, const dmx_site_fit_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_site_fit: null argument");
  const char* fn = "dmx_engine_site_fit";
  if (int rc = require_staged(e, fn)) return rc;
  const int32_t B = e->pv.B, V = e->V, S = e->S, M = rq->max_reads;
  if (int rc = require_sizes(e, fn, rq->n_cells, rq->n_snps)) return rc;
  if (M < 1 || M > kFitMaxReads) return set_error(DMX_ERR_ARG, "dmx_engine_site_fit: max_reads %d is not in [1, %d]", M, kFitMaxReads);
  HypPlan pl{fn, B, V, S, rq->hyp, rq->hyp_memory, rq->alpha, rq->rho, rq->ambient};
  if (int rc = pl.check_args()) return rc;
  const size_t per_chunk = sizeof(SitePartial) * (size_t)S;
  if (rq->partial_bytes < 0 || (rq->partial_bytes > 0 && (uint64_t)rq->partial_bytes < per_chunk))
    return set_error(DMX_ERR_ARG, "dmx_engine_site_fit: partial_bytes %lld is below one chunk's %zu bytes", (long long)rq->partial_bytes, per_chunk);
  if (int rc = pl.check_ranges()) return rc;
  HIP_TRY(hipSetDevice(e->device));
  if (int rc = pl.fetch(e)) return rc;
  if (int rc = pl.list()) return rc;
  const std::vector<int32_t>& idx = pl.idx;
  const int32_t n_sng = pl.n_sng, n_used = pl.n_used(), n_dbl = pl.n_dbl();
  // ---- plan: chunk_beg[nch + 1] | members[n_used]; no chunk straddles the two lists
  const int32_t ncs = (n_sng + kSiteChunk - 1) / kSiteChunk, ncd = (n_dbl + kSiteChunk - 1) / kSiteChunk, nch = ncs + ncd;
  std::vector<int32_t> plan;
  plan.reserve((size_t)nch + 1 + (size_t)n_used);
  for (int32_t c = 0; c < ncs; ++c) plan.push_back(c * kSiteChunk);
  for (int32_t c = 0; c < ncd; ++c) plan.push_back(n_sng + c * kSiteChunk);
  plan.push_back(n_used);                                             // (the last singlet chunk ends at chunk_beg[ncs] = n_sng either way)
  plan.insert(plan.end(), idx.begin(), idx.end());
  const size_t o_mem = (size_t)nch + 1;

  const int32_t nblk = (int32_t)(((int64_t)S + kRefSlab - 1) >> kRefSlabShift);
  const size_t out_b = sizeof(double) * 5 * (size_t)S, cnt_b = sizeof(int32_t) * 5 * (size_t)S, par_b = sizeof(double) * 2 * (size_t)B;
  const size_t blk_b = sizeof(int64_t) * 2 * (size_t)B * ((size_t)nblk + 1);
  const bool build_blk = !e->rblk_valid || e->rblk_S != S;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const size_t budget = rq->partial_bytes > 0 ? (size_t)rq->partial_bytes : std::min<size_t>((size_t)4 << 30, free_b / 6);
  const int32_t cpw = (int32_t)std::max<size_t>(1, std::min<size_t>({per_chunk ? budget / per_chunk : (size_t)65535, (size_t)65535, (size_t)std::max(nch, 1)}));
  const size_t part_b = nch > 0 ? per_chunk * (size_t)cpw : 0;
  const size_t need = out_b + cnt_b + par_b + sizeof(int32_t) * 2 * (size_t)B + sizeof(int32_t) * plan.size() + sizeof(double) * (size_t)S + part_b;
  const size_t grow = (out_b > e->d_sout.cap() ? need - part_b : 0) + (part_b > e->d_spart.cap() ? part_b : 0) +
                      (build_blk && blk_b > e->d_rblk.cap() ? blk_b : 0);
  if (grow && grow + grow / 16 > free_b)
    return set_error(DMX_ERR_NOMEM, "dmx_engine_site_fit: the results and partials of %d SNPs need %zu more bytes, %zu are free", S, grow, free_b);
  if (int rc = e->d_sout.ensure(out_b)) return rc;
  if (int rc = e->d_scnt.ensure(cnt_b)) return rc;
  if (int rc = e->d_spar.ensure(par_b)) return rc;
  if (int rc = e->d_shyp.ensure(sizeof(int32_t) * 2 * (size_t)B)) return rc;
  if (int rc = e->d_splan.ensure(sizeof(int32_t) * plan.size())) return rc;
  if (int rc = e->d_samb.ensure(sizeof(double) * (size_t)S)) return rc;
  if (part_b) if (int rc = e->d_spart.ensure(part_b)) return rc;
  if (build_blk && B > 0) if (int rc = e->d_rblk.ensure(blk_b)) return rc;
  e->have_site = false;
  if (int rc = pl.upload(e, e->d_shyp, e->d_spar)) return rc;
  HIP_TRY(hipMemcpyAsync(e->d_splan, plan.data(), sizeof(int32_t) * plan.size(), hipMemcpyHostToDevice, e->stream));
  if (S > 0) {
    HIP_TRY(hipMemsetAsync(e->d_sout, 0, out_b, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_scnt, 0, cnt_b, e->stream));
  }
  if (int rc = stage_soup(e, rq->ambient, S, e->d_samb)) return rc;
  if (build_blk && B > 0) {
    hipLaunchKernelGGL(k_snp_blocks, dim3((unsigned)((B + 3) / 4)), dim3(kThreads), 0, e->stream, e->pv, e->nrd_width, kRefSlabShift, nblk, e->d_rblk);
    HIP_TRY(hipGetLastError());
  }
  e->rblk_valid = true; e->rblk_S = S;
  const int32_t MMsel = M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : 8;
  int32_t n_waves = 0;
  if (int rc = e->siev.record_start(e->stream)) return rc;
  if (nch > 0 && S > 0) {
    const int32_t* d_beg = e->d_splan;
    const int32_t* d_mem = e->d_splan + o_mem;
    for (int32_t c0 = 0; c0 < nch; c0 += cpw, ++n_waves) {
      const int32_t c1 = std::min(c0 + cpw, nch), cs1 = std::min(c1, ncs), cd0 = std::max(c0, ncs);
      launch_site_partial<false>(e, MMsel, nblk, d_mem, d_beg, c0, cs1 - c0, 0, M);
      HIP_TRY(hipGetLastError());
      launch_site_partial<true>(e, MMsel, nblk, d_mem, d_beg, cd0, c1 - cd0, cd0 - c0, M);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_site_fold, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, e->stream, (const SitePartial*)e->d_spart.get(), S, c1 - c0,
                         e->d_sout.get(), e->d_scnt.get());
      HIP_TRY(hipGetLastError());
    }
  }
  if (int rc = e->siev.record_stop(e->stream)) return rc;
  std::vector<int32_t> tz((size_t)S * 2);
  if (S > 0) HIP_TRY(hipMemcpyAsync(tz.data(), e->d_scnt + 3 * (size_t)S, sizeof(int32_t) * 2 * (size_t)S, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));        // the caller's inputs may go away after return
  float ms = 0.f;
  if (int rc = e->siev.elapsed_ms(&ms)) return rc;
  dmx_site_fit_info& inf = e->site_info;
  std::memset(&inf, 0, sizeof inf);
  inf.kernel_ms = ms; inf.bytes = (int64_t)need; inf.partial_bytes = (int64_t)part_b;
  inf.n_chunks = nch; inf.n_waves = n_waves; inf.chunk_cells = kSiteChunk; inf.slab_snps = kRefSlab;
  inf.n_cells = B; inf.n_snps = S; inf.n_used = n_used; inf.n_singlet = n_sng; inf.n_doublet = n_dbl; inf.max_reads = M;
  for (int32_t i = 0; i < S; ++i) { inf.n_trunc += tz[(size_t)i]; inf.n_zero += tz[(size_t)S + i]; }
  e->site_S = S; e->have_site = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_site_fit(dmx_engine* e, double* obs, double* mean, double* var, double* exc, double* vexc, int32_t* n_cell,
                                       int32_t* n_read, int32_t* n_alt, int32_t* n_trunc, int32_t* n_zero) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_site_fit: null engine");
  if (!e->have_site) return set_error(DMX_ERR_STATE, "dmx_engine_get_site_fit: no result on the staged pileup (dmx_engine_site_fit first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t S = (size_t)e->site_S;
  if (!S) return DMX_OK;
  double* const dp[5] = {obs, mean, var, exc, vexc};
  int32_t* const ip[5] = {n_cell, n_read, n_alt, n_trunc, n_zero};
  for (int k = 0; k < 5; ++k)
    if (dp[k]) HIP_TRY(hipMemcpy(dp[k], e->d_sout + k * S, sizeof(double) * S, hipMemcpyDeviceToHost));
  for (int k = 0; k < 5; ++k)
    if (ip[k]) HIP_TRY(hipMemcpy(ip[k], e->d_scnt + k * S, sizeof(int32_t) * S, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_site_fit_info(dmx_engine* e, dmx_site_fit_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_site_fit_info: null argument");
  if (!e->have_site) return set_error(DMX_ERR_STATE, "dmx_engine_site_fit_info: no result on the staged pileup (dmx_engine_site_fit first)");
  *out = e->site_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Model-drawn null pool (csrc/dmx_redraw.hpp): dmx_engine_fit's checks and list of used barcodes, a device copy of
// the whole read array into the output, -1 into geno, and one launch of k_redraw over the used barcodes.
#include "dmx_redraw.hpp"

extern "C" int dmx_engine_redraw(dmx_engine* e, const dmx_redraw_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_redraw: null argument");
  const char* fn = "dmx_engine_redraw";
  if (int rc = require_staged(e, fn)) return rc;
  const int32_t B = e->pv.B, V = e->V, S = e->S;
  if ((e->d_rwreads && e->pv.reads == (const uint8_t*)e->d_rwreads.get()) || (e->d_cmpoff && e->pv.cell_pair_off == (const int64_t*)e->d_cmpoff.get()))
    return set_error(DMX_ERR_STATE, "dmx_engine_redraw: the staged pileup is this engine's own redrawn or composed pileup (it would be overwritten)");
  if (int rc = require_sizes(e, fn, rq->n_cells, rq->n_snps)) return rc;
  if (rq->genotype_draw != DMX_REDRAW_PAIR && rq->genotype_draw != DMX_REDRAW_DONOR)
    return set_error(DMX_ERR_ARG, "dmx_engine_redraw: genotype_draw %d is neither DMX_REDRAW_PAIR nor DMX_REDRAW_DONOR", rq->genotype_draw);
  if (rq->index_base < 0) return set_error(DMX_ERR_ARG, "dmx_engine_redraw: index_base %lld is negative", (long long)rq->index_base);
  HypPlan pl{fn, B, V, S, rq->hyp, rq->hyp_memory, rq->alpha, rq->rho, rq->ambient};
  if (int rc = pl.check_args()) return rc;
  if (int rc = pl.check_ranges()) return rc;
  HIP_TRY(hipSetDevice(e->device));
  std::vector<int64_t> h_po((size_t)B + 1, 0), h_ro((size_t)B + 1, 0);
  if (int rc = pl.fetch(e, /*sync=*/false)) return rc;   // (one synchronise for hyp and the two offset arrays)
  HIP_TRY(hipMemcpyAsync(h_po.data(), e->pv.cell_pair_off, sizeof(int64_t) * ((size_t)B + 1), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(h_ro.data(), e->pv.cell_read_off, sizeof(int64_t) * ((size_t)B + 1), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (int rc = pl.list()) return rc;
  const std::vector<int32_t>& idx = pl.idx;
  const int32_t n_sng = pl.n_sng, n_used = pl.n_used(), n_dbl = pl.n_dbl();
  // the view's extent: offsets are absolute in a view of a caller's device arrays, so the arrays reach to the last cell's end
  const int64_t P = h_po[(size_t)B], R = e->pv.R;
  if (P < 0 || R < 0 || h_ro[(size_t)B] > R) return set_error(DMX_ERR_STATE, "dmx_engine_redraw: the staged offsets leave the read array");
  const size_t reads_b = (size_t)R + 64, geno_b = 2 * (size_t)P + 16;   // (slack: the lean K1 reads four bytes at a time)
  const size_t cnt_b = sizeof(int32_t) * 4 * (size_t)B, par_b = sizeof(double) * 2 * (size_t)B;
  const size_t need = reads_b + geno_b + cnt_b + par_b + sizeof(int32_t) * 3 * (size_t)B + sizeof(double) * (size_t)S;
  {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t have = e->d_rwreads.cap() + e->d_rwgeno.cap();
    if ((reads_b > e->d_rwreads.cap() || geno_b > e->d_rwgeno.cap()) && need + need / 8 > free_b + have)
      return set_error(DMX_ERR_NOMEM, "dmx_engine_redraw: %lld read bytes and %lld pairs need %zu bytes, %zu are free", (long long)R, (long long)P, need, free_b);
  }
  e->have_redraw = false;
  if (int rc = e->d_rwreads.ensure(reads_b)) return rc;
  if (int rc = e->d_rwgeno.ensure(geno_b)) return rc;
  if (int rc = e->d_rwcnt.ensure(cnt_b)) return rc;
  if (int rc = e->d_rwpar.ensure(par_b)) return rc;
  if (int rc = e->d_rwhyp.ensure(sizeof(int32_t) * 2 * (size_t)B)) return rc;
  if (int rc = e->d_rwidx.ensure(sizeof(int32_t) * (size_t)B)) return rc;
  if (int rc = e->d_rwamb.ensure(sizeof(double) * (size_t)S)) return rc;
  if (int rc = pl.upload(e, e->d_rwhyp, e->d_rwpar)) return rc;
  if (B > 0) HIP_TRY(hipMemsetAsync(e->d_rwcnt, 0, cnt_b, e->stream));
  if (n_used > 0) HIP_TRY(hipMemcpyAsync(e->d_rwidx, idx.data(), sizeof(int32_t) * (size_t)n_used, hipMemcpyHostToDevice, e->stream));
  if (int rc = stage_soup(e, rq->ambient, S, e->d_rwamb)) return rc;
  // unused barcodes, pairs without stored reads, skipped pairs and kept reads: a plain copy of everything, which the kernel then overwrites
  if (R > 0) HIP_TRY(hipMemcpyAsync(e->d_rwreads, e->pv.reads, (size_t)R, hipMemcpyDeviceToDevice, e->stream));
  HIP_TRY(hipMemsetAsync(e->d_rwgeno, 0xFF, geno_b, e->stream));
  dmx_rdw::Ctx c{};
  c.pv = e->pv; c.nrd_width = e->nrd_width; c.tabs = (const double*)e->d_lut; c.g = e->d_g; c.V = V;
  c.idx = e->d_rwidx; c.n_idx = n_used; c.hyp = e->d_rwhyp; c.alpha = e->d_rwpar; c.rho = e->d_rwpar + B; c.amb = e->d_rwamb;
  c.seed = rq->seed; c.geno_seed = rq->geno_seed; c.index_base = rq->index_base; c.donor_draw = rq->genotype_draw == DMX_REDRAW_DONOR;
  c.B = B; c.o_reads = e->d_rwreads; c.o_geno = e->d_rwgeno; c.cnt = e->d_rwcnt;
  if (int rc = e->rwev.record_start(e->stream)) return rc;
  if (n_used > 0) {
    hipLaunchKernelGGL(dmx_rdw::k_redraw, dim3((unsigned)((n_used + dmx_rdw::kWaves - 1) / dmx_rdw::kWaves)), dim3(64 * dmx_rdw::kWaves), 0, e->stream, c);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->rwev.record_stop(e->stream)) return rc;
  std::vector<int32_t> cnt((size_t)B * 4);
  if (B > 0) HIP_TRY(hipMemcpyAsync(cnt.data(), e->d_rwcnt, cnt_b, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));        // the caller's inputs may go away after return
  float ms = 0.f;
  if (int rc = e->rwev.elapsed_ms(&ms)) return rc;
  dmx_redraw_info& inf = e->redraw_info;
  std::memset(&inf, 0, sizeof inf);
  inf.kernel_ms = ms; inf.n_cells = B; inf.n_used = n_used; inf.n_singlet = n_sng; inf.n_doublet = n_dbl; inf.genotype_draw = rq->genotype_draw;
  const int64_t pair_bytes = (e->pv.pair_snp ? 4 : 0) + e->nrd_width;
  for (int32_t k = 0; k < n_used; ++k) {
    const size_t b = (size_t)idx[(size_t)k];
    const int64_t drawn = cnt[b], skipped = cnt[(size_t)B + b], rd = cnt[2 * (size_t)B + b], rk = cnt[3 * (size_t)B + b];
    inf.n_pairs_drawn += drawn; inf.n_pairs_skipped += skipped; inf.n_reads_drawn += rd; inf.n_reads_kept += rk;
    inf.bytes_read += (h_po[b + 1] - h_po[b]) * pair_bytes + (drawn + skipped) * 12 * (k < n_sng ? 1 : 2) + rd + rk + 44;
    inf.bytes_written += rd + 2 * drawn + 16;
  }
  e->rw_pairs = P; e->have_redraw = true;
  return DMX_OK;
}

extern "C" int dmx_engine_redrawn_pileup(dmx_engine* e, dmx_pileup* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_redrawn_pileup: null argument");
  if (!e->have_redraw) return set_error(DMX_ERR_STATE, "dmx_engine_redrawn_pileup: nothing redrawn on the staged pileup (dmx_engine_redraw first)");
  std::memset(out, 0, sizeof *out);
  out->n_cells = e->pv.B; out->n_snps = e->pv.S; out->n_pairs = e->rw_pairs; out->n_reads = e->pv.R;
  out->cell_pair_off = e->pv.cell_pair_off; out->cell_read_off = e->pv.cell_read_off;
  out->pair_snp = e->pv.pair_snp; out->pair_nrd = e->pv.pair_nrd; out->nrd_width = e->nrd_width;
  out->memory = DMX_MEM_DEVICE; out->reads = e->d_rwreads;
  return DMX_OK;
}

extern "C" int dmx_engine_get_redrawn(dmx_engine* e, uint8_t* reads, int8_t* geno) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_redrawn: null engine");
  if (!e->have_redraw) return set_error(DMX_ERR_STATE, "dmx_engine_get_redrawn: nothing redrawn on the staged pileup (dmx_engine_redraw first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (reads && e->pv.R) HIP_TRY(hipMemcpy(reads, e->d_rwreads, (size_t)e->pv.R, hipMemcpyDeviceToHost));
  if (geno && e->rw_pairs) HIP_TRY(hipMemcpy(geno, e->d_rwgeno, 2 * (size_t)e->rw_pairs, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_redraw_info(dmx_engine* e, dmx_redraw_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_redraw_info: null argument");
  if (!e->have_redraw) return set_error(DMX_ERR_STATE, "dmx_engine_redraw_info: nothing redrawn on the staged pileup (dmx_engine_redraw first)");
  *out = e->redraw_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Continuous mixing share: both calls check their arguments on the host (anchors / cand, rho and a are small),
// copy them to buffers of their own and launch one kernel.
extern "C" int dmx_engine_share_scan(dmx_engine* e, const dmx_share_scan_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_share_scan: null argument");
  const char* fn = "dmx_engine_share_scan";
  if (int rc = require_staged(e, fn)) return rc;
  const int32_t B = e->pv.B, V = e->V, S = e->S, T = rq->n_anchor;
  if (int rc = require_sizes(e, fn, rq->n_cells, rq->n_snps)) return rc;
  if (T < 1 || T > kShareMaxAnchor) return set_error(DMX_ERR_ARG, "dmx_engine_share_scan: n_anchor %d is not in [1, %d]", T, kShareMaxAnchor);
  if (V > kShareMaxSamples) return set_error(DMX_ERR_ARG, "dmx_engine_share_scan: %d samples, at most %d", V, kShareMaxSamples);
  if (B > 0 && !rq->anchors) return set_error(DMX_ERR_ARG, "dmx_engine_share_scan: missing anchors");
  if (rq->rho && !rq->ambient && S > 0) return set_error(DMX_ERR_ARG, "dmx_engine_share_scan: rho is given without ambient");
  if (rq->anchor_memory != DMX_MEM_HOST && rq->anchor_memory != DMX_MEM_DEVICE)
    return set_error(DMX_ERR_ARG, "dmx_engine_share_scan: anchor_memory %d", rq->anchor_memory);
  if (int rc = check_unit_interval(fn, "rho", rq->rho, B)) return rc;
  if (int rc = check_unit_interval(fn, "ambient", rq->ambient, S)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  const size_t n_slot = (size_t)B * (size_t)T;
  std::vector<int32_t> an;
  if (int rc = fetch_ids(e, rq->anchors, rq->anchor_memory, n_slot, an)) return rc;
  int64_t n_used = 0;
  for (size_t k = 0; k < n_slot; ++k) {
    if (an[k] == -1) continue;
    if (an[k] < 0 || an[k] >= V)
      return set_error(DMX_ERR_ARG, "dmx_engine_share_scan: anchors[%zu][%zu] = %d is not -1 or a sample in [0, %d)", k / (size_t)T, k % (size_t)T, an[k], V);
    ++n_used;
  }
  const size_t out_b = sizeof(double) * 3 * n_slot * (size_t)V, cnt_b = sizeof(int32_t) * 2 * n_slot;
  const size_t need = out_b + cnt_b + sizeof(int32_t) * n_slot + sizeof(double) * ((size_t)B + (size_t)S);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (out_b > e->d_ssout.cap() && need + need / 16 > free_b)
    return set_error(DMX_ERR_NOMEM, "dmx_engine_share_scan: the %d x %d x %d scan needs %zu bytes, %zu are free", B, T, V, need, free_b);
  if (int rc = e->d_ssout.ensure(out_b)) return rc;
  if (int rc = e->d_sscnt.ensure(cnt_b)) return rc;
  if (int rc = e->d_ssanc.ensure(sizeof(int32_t) * n_slot)) return rc;
  if (int rc = e->d_ssrho.ensure(sizeof(double) * (size_t)B)) return rc;
  if (int rc = e->d_ssamb.ensure(sizeof(double) * (size_t)S)) return rc;
  e->have_sscan = false;
  if (int rc = stage_soup(e, rq->rho, B, e->d_ssrho)) return rc;
  if (int rc = stage_soup(e, rq->ambient, S, e->d_ssamb)) return rc;
  if (n_slot > 0) {
    HIP_TRY(hipMemcpyAsync(e->d_ssanc, an.data(), sizeof(int32_t) * n_slot, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_ssout, 0, out_b, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_sscnt, 0, cnt_b, e->stream));
  }
  const int32_t n_vblk = (V + 63) / 64;
  const int64_t n_units = (int64_t)n_slot * n_vblk;
  if (int rc = e->ssev.record_start(e->stream)) return rc;
  if (n_units > 0) {
    hipLaunchKernelGGL(k_share_scan, dim3((unsigned)((n_units + kShareWaves - 1) / kShareWaves)), dim3(64 * kShareWaves), 0, e->stream, e->pv,
                       e->nrd_width, (const double*)e->d_lut, e->d_g, V, (const int32_t*)e->d_ssanc, T, (const double*)e->d_ssrho,
                       (const double*)e->d_ssamb, n_vblk, n_units, e->d_ssout.get(), e->d_sscnt.get());
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->ssev.record_stop(e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));        // the caller's inputs may go away after return
  float ms = 0.f;
  if (int rc = e->ssev.elapsed_ms(&ms)) return rc;
  dmx_share_info& inf = e->share_info;
  inf.scan_ms = ms; inf.scan_bytes = (int64_t)need; inf.scan_entries = n_used * (int64_t)(V - 1);
  inf.n_cells = B; inf.n_samples = V; inf.n_anchor = T; inf.have_scan = 1;
  e->ss_B = B; e->ss_T = T; e->ss_V = V; e->have_sscan = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_share_scan(dmx_engine* e, double* out, int32_t* n_snp_read) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_share_scan: null engine");
  if (!e->have_sscan) return set_error(DMX_ERR_STATE, "dmx_engine_get_share_scan: no scan on the staged pileup (dmx_engine_share_scan first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t n_slot = (size_t)e->ss_B * (size_t)e->ss_T;
  if (!n_slot) return DMX_OK;
  if (out) HIP_TRY(hipMemcpy(out, e->d_ssout, sizeof(double) * 3 * n_slot * (size_t)e->ss_V, hipMemcpyDeviceToHost));
  if (n_snp_read) HIP_TRY(hipMemcpy(n_snp_read, e->d_sscnt, sizeof(int32_t) * 2 * n_slot, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_share_fit(dmx_engine* e, const dmx_share_fit_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_share_fit: null argument");
  const char* fn = "dmx_engine_share_fit";
  if (int rc = require_staged(e, fn)) return rc;
  const int32_t B = e->pv.B, V = e->V, S = e->S, C = rq->n_cand;
  if (int rc = require_sizes(e, fn, rq->n_cells, rq->n_snps)) return rc;
  if (C < 1 || C > kShareMaxCand) return set_error(DMX_ERR_ARG, "dmx_engine_share_fit: n_cand %d is not in [1, %d]", C, kShareMaxCand);
  if (B > 0 && !rq->cand) return set_error(DMX_ERR_ARG, "dmx_engine_share_fit: missing cand");
  if (rq->rho && !rq->ambient && S > 0) return set_error(DMX_ERR_ARG, "dmx_engine_share_fit: rho is given without ambient");
  if (rq->cand_memory != DMX_MEM_HOST && rq->cand_memory != DMX_MEM_DEVICE) return set_error(DMX_ERR_ARG, "dmx_engine_share_fit: cand_memory %d", rq->cand_memory);
  if (!(rq->tol > 0.0 && rq->tol < INFINITY)) return set_error(DMX_ERR_ARG, "dmx_engine_share_fit: tol %g is not a positive number", rq->tol);
  if (rq->max_iter < 1 || rq->max_iter > kShareMaxIter) return set_error(DMX_ERR_ARG, "dmx_engine_share_fit: max_iter %d is not in [1, %d]", rq->max_iter, kShareMaxIter);
  if (!(rq->start > 0.0 && rq->start < 1.0)) return set_error(DMX_ERR_ARG, "dmx_engine_share_fit: start %g is not in (0, 1)", rq->start);
  if (!(rq->probe < 0.0 || (rq->probe >= 0.0 && rq->probe <= 1.0)))
    return set_error(DMX_ERR_ARG, "dmx_engine_share_fit: probe %g is neither negative (none) nor in [0, 1]", rq->probe);
  if (int rc = check_unit_interval(fn, "rho", rq->rho, B)) return rc;
  if (int rc = check_unit_interval(fn, "ambient", rq->ambient, S)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  const size_t n_slot = (size_t)B * (size_t)C;
  std::vector<int32_t> cd;
  if (int rc = fetch_ids(e, rq->cand, rq->cand_memory, 2 * n_slot, cd)) return rc;
  int64_t n_used = 0;
  if (int rc = check_pairs(fn, "cand", cd, n_slot, C, V, &n_used)) return rc;
  const size_t out_b = sizeof(double) * kShareFitDoubles * n_slot, int_b = sizeof(int32_t) * kShareFitInts * n_slot;
  const size_t need = out_b + int_b + sizeof(int32_t) * 2 * n_slot + sizeof(double) * ((size_t)B + (size_t)S);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (out_b > e->d_sfout.cap() && need + need / 16 > free_b)
    return set_error(DMX_ERR_NOMEM, "dmx_engine_share_fit: the results of %d x %d candidates need %zu bytes, %zu are free", B, C, need, free_b);
  if (int rc = e->d_sfout.ensure(out_b)) return rc;
  if (int rc = e->d_sfint.ensure(int_b)) return rc;
  if (int rc = e->d_sfcand.ensure(sizeof(int32_t) * 2 * n_slot)) return rc;
  if (int rc = e->d_sfrho.ensure(sizeof(double) * (size_t)B)) return rc;
  if (int rc = e->d_sfamb.ensure(sizeof(double) * (size_t)S)) return rc;
  e->have_sfit = false;
  if (int rc = stage_soup(e, rq->rho, B, e->d_sfrho)) return rc;
  if (int rc = stage_soup(e, rq->ambient, S, e->d_sfamb)) return rc;
  if (n_slot > 0) {
    HIP_TRY(hipMemcpyAsync(e->d_sfcand, cd.data(), sizeof(int32_t) * 2 * n_slot, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_sfout, 0, out_b, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_sfint, 0, int_b, e->stream));
  }
  const int64_t n_units = (int64_t)n_slot;
  if (int rc = e->sfev.record_start(e->stream)) return rc;
  if (n_units > 0) {
    hipLaunchKernelGGL(k_share_fit, dim3((unsigned)((n_units + kShareWaves - 1) / kShareWaves)), dim3(64 * kShareWaves), 0, e->stream, e->pv,
                       e->nrd_width, (const double*)e->d_lut, e->d_g, V, (const int32_t*)e->d_sfcand, (const double*)e->d_sfrho,
                       (const double*)e->d_sfamb, rq->start, rq->tol, rq->max_iter, rq->probe, n_units, e->d_sfout.get(), e->d_sfint.get());
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->sfev.record_stop(e->stream)) return rc;
  std::vector<int32_t> oi(kShareFitInts * n_slot);
  if (n_slot > 0) HIP_TRY(hipMemcpyAsync(oi.data(), e->d_sfint, int_b, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));        // the caller's inputs may go away after return
  float ms = 0.f;
  if (int rc = e->sfev.elapsed_ms(&ms)) return rc;
  dmx_share_info& inf = e->share_info;
  inf.fit_ms = ms; inf.fit_bytes = (int64_t)need; inf.fit_used = n_used; inf.fit_evals = 0;
  for (size_t k = 0; k < n_slot; ++k)
    if (cd[2 * k] >= 0) inf.fit_evals += oi[kShareFitInts * k] + (rq->probe >= 0.0 ? 1 : 0);
  inf.n_cells = B; inf.n_samples = V; inf.n_cand = C; inf.have_fit = 1;
  e->sf_B = B; e->sf_C = C; e->have_sfit = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_share_fit(dmx_engine* e, double* values, int32_t* counts) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_share_fit: null engine");
  if (!e->have_sfit) return set_error(DMX_ERR_STATE, "dmx_engine_get_share_fit: no fit on the staged pileup (dmx_engine_share_fit first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t n_slot = (size_t)e->sf_B * (size_t)e->sf_C;
  if (!n_slot) return DMX_OK;
  if (values) HIP_TRY(hipMemcpy(values, e->d_sfout, sizeof(double) * kShareFitDoubles * n_slot, hipMemcpyDeviceToHost));
  if (counts) HIP_TRY(hipMemcpy(counts, e->d_sfint, sizeof(int32_t) * kShareFitInts * n_slot, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_share_info(dmx_engine* e, dmx_share_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_share_info: null argument");
  if (!e->have_sscan && !e->have_sfit)
    return set_error(DMX_ERR_STATE, "dmx_engine_share_info: neither call has run on the staged pileup (dmx_engine_share_scan / _share_fit first)");
  *out = e->share_info;
  out->have_scan = e->have_sscan; out->have_fit = e->have_sfit;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Joint genotype tables (csrc/dmx_kin.hpp): the arguments are checked on the host (the weight is small), host
// matrices are copied to buffers of the call's own, k_kin_rows runs once per side and k_kin_tile once.
#include "dmx_kin.hpp"

extern "C" int dmx_engine_geno_compare(dmx_engine* e, const dmx_kin_request* rq) {
  if (!e || !rq) return set_error(DMX_ERR_ARG, "dmx_engine_geno_compare: null argument");
  const int32_t S = rq->n_snps, VA = rq->n_a, VB = rq->n_b;
  if (VA < 1 || VA > DMX_KIN_MAX_COLUMNS) return set_error(DMX_ERR_ARG, "dmx_engine_geno_compare: n_a %d is not in [1, %d]", VA, DMX_KIN_MAX_COLUMNS);
  if (VB < 1 || VB > DMX_KIN_MAX_COLUMNS) return set_error(DMX_ERR_ARG, "dmx_engine_geno_compare: n_b %d is not in [1, %d]", VB, DMX_KIN_MAX_COLUMNS);
  if (S < 0) return set_error(DMX_ERR_ARG, "dmx_engine_geno_compare: n_snps %d is negative", S);
  if (rq->reserved != 0) return set_error(DMX_ERR_ARG, "dmx_engine_geno_compare: reserved is %d, not 0", rq->reserved);
  if (rq->g_memory != DMX_MEM_HOST && rq->g_memory != DMX_MEM_DEVICE) return set_error(DMX_ERR_ARG, "dmx_engine_geno_compare: g_memory %d", rq->g_memory);
  if (!rq->gb && VB != VA) return set_error(DMX_ERR_ARG, "dmx_engine_geno_compare: gb is NULL (B is A) but n_b %d is not n_a %d", VB, VA);
  if (!rq->ga) {
    if (!e->d_g) return set_error(DMX_ERR_STATE, "dmx_engine_geno_compare: ga is NULL and no genotype matrix is staged (dmx_engine_set_genotypes first)");
    if (e->S != S || e->V != VA)
      return set_error(DMX_ERR_STATE, "dmx_engine_geno_compare: ga is NULL and the staged matrix is %d x %d, the request says %d x %d", e->S, e->V, S, VA);
  }
  HIP_TRY(hipSetDevice(e->device));
  const bool on_host = rq->g_memory == DMX_MEM_HOST;
  if (rq->weight && S > 0) {
    std::vector<double> hw;
    const double* w = rq->weight;
    if (!on_host) {
      hw.resize((size_t)S);
      HIP_TRY(hipMemcpyAsync(hw.data(), rq->weight, sizeof(double) * (size_t)S, hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(hipStreamSynchronize(e->stream));
      w = hw.data();
    }
    for (int32_t i = 0; i < S; ++i)
      if (!(w[i] >= 0.0 && w[i] < INFINITY)) return set_error(DMX_ERR_ARG, "dmx_engine_geno_compare: weight[%d] = %g is not a finite number >= 0", i, w[i]);
  }
  const size_t na = (size_t)S * (size_t)VA, nb = (size_t)S * (size_t)VB;
  const size_t ga_b = rq->ga && on_host ? sizeof(float) * 3 * na : 0, gb_b = rq->gb && on_host ? sizeof(float) * 3 * nb : 0;
  const size_t w_b = rq->weight && on_host ? sizeof(double) * (size_t)S : 0;
  const size_t ia_b = sizeof(double) * 4 * na, ib_b = sizeof(double) * 4 * nb, tab_b = sizeof(double) * 16 * (size_t)VA * (size_t)VB;
  const size_t cnt_b = sizeof(int32_t) * ((size_t)VA + (size_t)VB);
  {
    size_t free_b = 0, total_b = 0, grow = 0, freed = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t want[7] = {ga_b, gb_b, w_b, ia_b, ib_b, tab_b, cnt_b};
    const size_t caps[7] = {e->d_knga.cap(), e->d_kngb.cap(), e->d_knw.cap(), e->d_knia.cap(), e->d_knib.cap(), e->d_knt.cap(), e->d_kncnt.cap()};
    for (int k = 0; k < 7; ++k)
      if (want[k] > caps[k]) { grow += want[k] + want[k] / 16 + 16; freed += caps[k]; }
    if (grow > free_b + freed)
      return set_error(DMX_ERR_NOMEM, "dmx_engine_geno_compare: %d SNPs x (%d + %d) columns need %zu bytes of matrices, %zu of images and %zu of table; %zu more than are held, %zu are free",
                       S, VA, VB, ga_b + gb_b + w_b, ia_b + ib_b, tab_b, grow, free_b);
  }
  e->have_kin = false;
  if (ga_b) if (int rc = e->d_knga.ensure(ga_b)) return rc;
  if (gb_b) if (int rc = e->d_kngb.ensure(gb_b)) return rc;
  if (w_b) if (int rc = e->d_knw.ensure(w_b)) return rc;
  if (int rc = e->d_knia.ensure(ia_b)) return rc;
  if (int rc = e->d_knib.ensure(ib_b)) return rc;
  if (int rc = e->d_knt.ensure(tab_b)) return rc;
  if (int rc = e->d_kncnt.ensure(cnt_b)) return rc;
  const float* d_ga = e->d_g;
  if (rq->ga) {
    d_ga = rq->ga;
    if (on_host) {
      if (na > 0) HIP_TRY(hipMemcpyAsync(e->d_knga, rq->ga, ga_b, hipMemcpyHostToDevice, e->stream));
      d_ga = e->d_knga;
    }
  }
  const float* d_gb = d_ga;
  if (rq->gb) {
    d_gb = rq->gb;
    if (on_host) {
      if (nb > 0) HIP_TRY(hipMemcpyAsync(e->d_kngb, rq->gb, gb_b, hipMemcpyHostToDevice, e->stream));
      d_gb = e->d_kngb;
    }
  }
  const double* d_w = nullptr;
  if (rq->weight && S > 0) {
    d_w = rq->weight;
    if (on_host) {
      HIP_TRY(hipMemcpyAsync(e->d_knw, rq->weight, w_b, hipMemcpyHostToDevice, e->stream));
      d_w = e->d_knw;
    }
  }
  HIP_TRY(hipMemsetAsync(e->d_kncnt, 0, cnt_b, e->stream));
  if (int rc = e->knrev.record_start(e->stream)) return rc;
  if (na > 0) {
    const unsigned ga_grid = (unsigned)std::min<size_t>((na + 255) / 256, (size_t)1 << 20), gb_grid = (unsigned)std::min<size_t>((nb + 255) / 256, (size_t)1 << 20);
    hipLaunchKernelGGL(dmx_kin::k_kin_rows, dim3(ga_grid), dim3(256), 0, e->stream, d_ga, (int64_t)na, VA, d_w, e->d_knia.get(), e->d_kncnt.get());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(dmx_kin::k_kin_rows, dim3(gb_grid), dim3(256), 0, e->stream, d_gb, (int64_t)nb, VB, (const double*)nullptr, e->d_knib.get(),
                       e->d_kncnt.get() + VA);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->knrev.record_stop(e->stream)) return rc;
  // the wide block where its tiling alone fills the chip; the bits are the same either way
  const bool wide = (int64_t)((VA + 31) / 32) * ((VB + 31) / 32) >= dmx_kin::kWideTiles;
  const int32_t tile = wide ? 32 : 16;
  const dim3 grid((unsigned)((VB + tile - 1) / tile), (unsigned)((VA + tile - 1) / tile));
  const int32_t chunk = wide ? dmx_kin::kChunkWide : dmx_kin::kChunkNarrow;
  const size_t lds_b = 2 * (size_t)(2 * chunk * 2 * tile) * 16;
  if (int rc = e->kntev.record_start(e->stream)) return rc;
  if (wide)
    hipLaunchKernelGGL((dmx_kin::k_kin_tile<2, 2, dmx_kin::kChunkWide>), grid, dim3(dmx_kin::kThreads), lds_b, e->stream, (const double*)e->d_knia, (const double*)e->d_knib, S, VA, VB, e->d_knt.get());
  else
    hipLaunchKernelGGL((dmx_kin::k_kin_tile<1, 1, dmx_kin::kChunkNarrow>), grid, dim3(dmx_kin::kThreads), lds_b, e->stream, (const double*)e->d_knia, (const double*)e->d_knib, S, VA, VB, e->d_knt.get());
  HIP_TRY(hipGetLastError());
  if (int rc = e->kntev.record_stop(e->stream)) return rc;
  e->kn_invalid.assign((size_t)VA + (size_t)VB, 0);
  HIP_TRY(hipMemcpyAsync(e->kn_invalid.data(), e->d_kncnt, cnt_b, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));        // the caller's inputs may go away after return
  float ms_r = 0.f, ms_t = 0.f;
  if (int rc = e->knrev.elapsed_ms(&ms_r)) return rc;
  if (int rc = e->kntev.elapsed_ms(&ms_t)) return rc;
  dmx_kin_info& inf = e->kin_info;
  std::memset(&inf, 0, sizeof inf);
  inf.rows_ms = ms_r; inf.tile_ms = ms_t;
  inf.flop = 2 * 16 * (int64_t)VA * (int64_t)VB * (int64_t)S;
  inf.bytes = (int64_t)(sizeof(float) * 3 * (na + nb) + (d_w ? sizeof(double) * (size_t)S : 0) + 2 * (ia_b + ib_b) + tab_b);
  for (int32_t v = 0; v < VA; ++v) inf.n_invalid_a += e->kn_invalid[(size_t)v];
  for (int32_t v = 0; v < VB; ++v) inf.n_invalid_b += e->kn_invalid[(size_t)VA + v];
  inf.n_snps = S; inf.n_a = VA; inf.n_b = VB; inf.tile_a = tile; inf.tile_b = tile; inf.chunk_snps = chunk;
  e->have_kin = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_geno_compare(dmx_engine* e, double* table, int32_t* n_valid_a, int32_t* n_valid_b) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_geno_compare: null engine");
  if (!e->have_kin) return set_error(DMX_ERR_STATE, "dmx_engine_get_geno_compare: nothing compared yet (dmx_engine_geno_compare first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const dmx_kin_info& inf = e->kin_info;
  if (table) HIP_TRY(hipMemcpy(table, e->d_knt, sizeof(double) * 16 * (size_t)inf.n_a * (size_t)inf.n_b, hipMemcpyDeviceToHost));
  if (n_valid_a) for (int32_t v = 0; v < inf.n_a; ++v) n_valid_a[v] = inf.n_snps - e->kn_invalid[(size_t)v];
  if (n_valid_b) for (int32_t v = 0; v < inf.n_b; ++v) n_valid_b[v] = inf.n_snps - e->kn_invalid[(size_t)inf.n_a + v];
  return DMX_OK;
}

extern "C" int dmx_engine_geno_compare_info(dmx_engine* e, dmx_kin_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_geno_compare_info: null argument");
  if (!e->have_kin) return set_error(DMX_ERR_STATE, "dmx_engine_geno_compare_info: nothing compared yet (dmx_engine_geno_compare first)");
  *out = e->kin_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Block-resolved likelihoods (csrc/dmx_blocks.hpp): block[] and extra[] are checked on the host and copied to
// buffers of the call's own, the results are zeroed, and k_block_col runs once over B x slabs wavefronts on the engine's stream.
#include "dmx_blocks.hpp"

extern "C" int dmx_engine_block_llk(dmx_engine* e, const dmx_block_llk_request* rq) {
  const char* fn = "dmx_engine_block_llk";
  if (!e || !rq) return set_error(DMX_ERR_ARG, "%s: null argument", fn);
  if (int rc = require_staged(e, fn)) return rc;
  if (int rc = require_sizes(e, fn, rq->n_cells, rq->n_snps)) return rc;
  const int32_t B = e->pv.B, S = e->S, V = e->V, A = e->A, G = rq->n_blocks, E = rq->n_extra;
  if (A > 64 || V > 0xFFE) return set_error(DMX_ERR_ARG, "%s: %d samples x %d alphas exceed this build's limits (4094 samples, 64 alphas)", fn, V, A);
  if (G < 1) return set_error(DMX_ERR_ARG, "%s: n_blocks %d is not at least 1", fn, G);
  if (E < 0 || E > dmx_blk::kMaxExtra) return set_error(DMX_ERR_ARG, "%s: n_extra %d is not in [0, %d]", fn, E, dmx_blk::kMaxExtra);
  for (int i = 0; i < 4; ++i)
    if (rq->reserved[i] != 0) return set_error(DMX_ERR_ARG, "%s: reserved[%d] = %d is not 0", fn, i, rq->reserved[i]);
  if (S > 0 && !rq->block) return set_error(DMX_ERR_ARG, "%s: block is null", fn);
  const size_t n_ex = (size_t)B * (size_t)E * 3;
  if (n_ex > 0 && !rq->extra) return set_error(DMX_ERR_ARG, "%s: extra is null with n_extra %d", fn, E);
  if (n_ex > 0 && rq->extra_memory != DMX_MEM_HOST && rq->extra_memory != DMX_MEM_DEVICE)
    return set_error(DMX_ERR_ARG, "%s: extra_memory %d", fn, rq->extra_memory);
  for (int32_t i = 0; i < S; ++i) {
    const int32_t g = rq->block[i];
    if (g < 0 || g >= G) return set_error(DMX_ERR_ARG, "%s: block[%d] = %d is not in [0, %d)", fn, i, g, G);
    if (i > 0 && g < rq->block[i - 1]) return set_error(DMX_ERR_ARG, "%s: block[%d] = %d decreases (block[%d] = %d)", fn, i, g, i - 1, rq->block[i - 1]);
  }
  if (!e->geno_rows_safe)
    return set_error(DMX_ERR_ARG, "%s: the genotype matrix has a row that is not finite, non-negative and above 1e-30 somewhere; the block pass has "
                                  "no fix-up pass for such a matrix (nor has the anchored search): repair or drop those rows first", fn);
  HIP_TRY(hipSetDevice(e->device));
  std::vector<int32_t> ex;
  int64_t n_used = 0;
  if (n_ex > 0) {
    if (int rc = fetch_ids(e, rq->extra, rq->extra_memory, n_ex, ex)) return rc;
    for (size_t b = 0; b < (size_t)B; ++b)
      for (int32_t s = 0; s < E; ++s) {
        const int32_t* x = &ex[(b * E + s) * 3];
        if (x[0] == -1) continue;
        if (x[0] < 0 || x[0] >= V || x[1] < 0 || x[1] >= V || x[2] < 0 || x[2] >= A)
          return set_error(DMX_ERR_ARG, "%s: extra[%zu][%d] = (%d, %d, %d) is not unused (j = -1) or an entry of [0, %d) x [0, %d) x [0, %d)", fn, b, s,
                           x[0], x[1], x[2], V, V, A);
        ++n_used;
      }
  }
  // the results: B G (V + A + E) doubles and B G counts
  const double want = (double)B * (double)G * ((double)(V + A + E) * sizeof(double) + sizeof(int32_t));
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (want > 0x1p60)
    return set_error(DMX_ERR_NOMEM, "%s: the results of %d barcodes x %d blocks x (%d + %d + %d) entries need %.3g bytes, %zu are free", fn, B, G, V, A,
                     E, want, free_b);
  const size_t BG = (size_t)B * (size_t)G;
  const size_t col_b = sizeof(double) * BG * V, l00_b = sizeof(double) * BG * A, ext_b = sizeof(double) * BG * E, n_b = sizeof(int32_t) * BG,
               blk_b = sizeof(int32_t) * (size_t)S, ex_b = sizeof(int32_t) * n_ex;
  const size_t need = (col_b > e->d_bkcol.cap() ? col_b + col_b / 16 : 0) + (l00_b > e->d_bkl00.cap() ? l00_b + l00_b / 16 : 0) +
                      (ext_b > e->d_bkext.cap() ? ext_b + ext_b / 16 : 0) + (n_b > e->d_bkn.cap() ? n_b + n_b / 16 : 0) +
                      (blk_b > e->d_bkblock.cap() ? blk_b + blk_b / 16 : 0) + (ex_b > e->d_bkextra.cap() ? ex_b + ex_b / 16 : 0);
  if (need > free_b)
    return set_error(DMX_ERR_NOMEM, "%s: the results of %d barcodes x %d blocks x (%d + %d + %d) entries need %zu bytes, %zu are free", fn, B, G, V, A, E,
                     col_b + l00_b + ext_b + n_b, free_b);
  e->have_blk = false;
  if (int rc = e->d_bkcol.ensure(col_b)) return rc;
  if (int rc = e->d_bkl00.ensure(l00_b)) return rc;
  if (int rc = e->d_bkext.ensure(ext_b)) return rc;
  if (int rc = e->d_bkn.ensure(n_b)) return rc;
  if (int rc = e->d_bkblock.ensure(blk_b)) return rc;
  if (int rc = e->d_bkextra.ensure(ex_b)) return rc;
  int A_pad = 1;
  while (A_pad < A) A_pad <<= 1;
  const int TP = std::min(dmx_blk::kTP, 64 / A_pad);
  const int32_t n_slab = (int32_t)((V + E + 63) / 64);
  const int64_t n_units = (int64_t)B * n_slab;
  if (S > 0) HIP_TRY(hipMemcpyAsync(e->d_bkblock, rq->block, blk_b, hipMemcpyHostToDevice, e->stream));
  if (n_ex > 0) HIP_TRY(hipMemcpyAsync(e->d_bkextra, ex.data(), ex_b, hipMemcpyHostToDevice, e->stream));
  if (int rc = e->bkzev.record_start(e->stream)) return rc;
  if (BG > 0) {
    HIP_TRY(hipMemsetAsync(e->d_bkcol, 0, col_b, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_bkl00, 0, l00_b, e->stream));
    if (ext_b > 0) HIP_TRY(hipMemsetAsync(e->d_bkext, 0, ext_b, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_bkn, 0, n_b, e->stream));
  }
  if (int rc = e->bkzev.record_stop(e->stream)) return rc;
  if (int rc = e->bkev.record_start(e->stream)) return rc;
  if (BG > 0) {
    hipLaunchKernelGGL(dmx_blk::k_block_col, dim3((unsigned)((n_units + dmx_blk::kWaves - 1) / dmx_blk::kWaves)), dim3(64 * dmx_blk::kWaves), 0, e->stream,
                       e->pv, e->nrd_width, e->d_g, (const double*)e->d_gp0, (const double*)e->d_lut, (const double*)e->d_alpha, V, A, A_pad, TP,
                       (const int32_t*)e->d_bkblock, G, (const int32_t*)e->d_bkextra, E, n_slab, n_units, e->d_bkcol.get(), e->d_bkl00.get(),
                       e->d_bkext.get(), e->d_bkn.get());
    HIP_TRY(hipGetLastError());
  }
  if (int rc = e->bkev.record_stop(e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));        // block[] and ex are pageable host memory that may go away after return
  dmx_block_llk_info& inf = e->blk_info;
  std::memset(&inf, 0, sizeof inf);
  float ms = 0.f;
  if (int rc = e->bkev.elapsed_ms(&ms)) return rc;
  inf.kernel_ms = ms;
  if (int rc = e->bkzev.elapsed_ms(&ms)) return rc;
  inf.zero_ms = ms;
  inf.result_bytes = (int64_t)(col_b + l00_b + ext_b + n_b);
  inf.n_entries = (int64_t)B * (V + A) + n_used;
  inf.n_cells = B; inf.n_samples = V; inf.n_alpha = A; inf.n_blocks = G; inf.n_extra = E;
  e->have_blk = true;
  return DMX_OK;
}

extern "C" int dmx_engine_get_block_llk(dmx_engine* e, double* col, double* l00, double* ext, int32_t* n_snp) {
  if (!e) return set_error(DMX_ERR_ARG, "dmx_engine_get_block_llk: null engine");
  if (!e->have_blk) return set_error(DMX_ERR_STATE, "dmx_engine_get_block_llk: no block result on the staged pileup (dmx_engine_block_llk first)");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const dmx_block_llk_info& inf = e->blk_info;
  const size_t BG = (size_t)inf.n_cells * (size_t)inf.n_blocks;
  if (!BG) return DMX_OK;
  if (col) HIP_TRY(hipMemcpy(col, e->d_bkcol, sizeof(double) * BG * (size_t)inf.n_samples, hipMemcpyDeviceToHost));
  if (l00) HIP_TRY(hipMemcpy(l00, e->d_bkl00, sizeof(double) * BG * (size_t)inf.n_alpha, hipMemcpyDeviceToHost));
  if (ext && inf.n_extra > 0) HIP_TRY(hipMemcpy(ext, e->d_bkext, sizeof(double) * BG * (size_t)inf.n_extra, hipMemcpyDeviceToHost));
  if (n_snp) HIP_TRY(hipMemcpy(n_snp, e->d_bkn, sizeof(int32_t) * BG, hipMemcpyDeviceToHost));
  return DMX_OK;
}

extern "C" int dmx_engine_block_llk_info(dmx_engine* e, dmx_block_llk_info* out) {
  if (!e || !out) return set_error(DMX_ERR_ARG, "dmx_engine_block_llk_info: null argument");
  if (!e->have_blk) return set_error(DMX_ERR_STATE, "dmx_engine_block_llk_info: no block result on the staged pileup (dmx_engine_block_llk first)");
  *out = e->blk_info;
  return DMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// BGZF members inflated on the device (csrc/dmx_gpu_inflate.hpp): k_bgzf_inflate and the dmx_inflater_* calls,
// independent of any engine.
#include "dmx_gpu_inflate.hpp"
