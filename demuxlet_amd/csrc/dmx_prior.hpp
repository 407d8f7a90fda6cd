// Empirical-Bayes priors from the doublet grid (dmx_engine_prior_step / _fit / _call): device code only,
// included by dmx_engine.hip.
//
// For barcode b with grid L[j][k][n] = llksAB[b][j][k][n] the USED entries are S_j = L[j][0][0] and D_jkn = L[j][k][n] for j != k, n >= 1.
//   w_S(j) = (1 - d) pi_j + d pi_j^2,  w_D(j,k,n) = d pi_j pi_k / (A - 1),
//   E_b = sum_j w_S(j) exp(S_j) + sum_{j != k, n >= 1} w_D(j,k,n) exp(D_jkn).
// One wavefront owns a barcode.  Every term is t = exp((L + log w) - m) with m the maximum of L + log w over the terms with w > 0 and
// L > -inf (pass 1, an order-free wave maximum); a term with w = 0 or L = -inf is exactly 0 and is never put through exp.  Pass 2 walks
// the rows j in ascending order; in a row lane l owns the slots e = l, l + 64, ... of the row's V A doubles (e = k A + n), so the loads
// are coalesced.  A slot's column accumulator lives in LDS and is touched by that lane alone: it adds the rows in ascending j.  A row's
// sum is the lane's slots in ascending e, then a butterfly over the 64 lanes (xor 1, 2, 4, ... 32).  The tail sums over j are serial in
// ascending j.  Nothing depends on the workgroup's width, the grid's address or the other barcodes.  No floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dmx.h"

namespace dmx_prior {

constexpr int kPriMaxVA = 4096;                  // V A: the shared table and one wavefront's slots, rows and singlets must fit the LDS
constexpr int kPriChunk = 64;                    // barcodes per chunk of the fold (section 12's convention)

// tab = log pi[V] | log w_S[V] | hf[V] | log(d / (A - 1)), hf_j = d pi_j / ((1 - d) + d pi_j) the homotypic part of a singlet-like term
__device__ inline void prior_tables(const double* __restrict__ pi, double d, int32_t V, int32_t A, double* __restrict__ tab, int tid, int nt) {
  for (int32_t j = tid; j < V; j += nt) {
    const double p = pi[j];
    const double ws = (1.0 - d) * p + (d * p) * p;
    const double den = (1.0 - d) + d * p;
    tab[j] = p > 0.0 ? log(p) : -INFINITY;
    tab[V + j] = ws > 0.0 ? log(ws) : -INFINITY;
    tab[2 * V + j] = (ws > 0.0 && den > 0.0) ? (d * p) / den : 0.0;
  }
  if (tid == 0) tab[3 * V] = d > 0.0 ? log(d / (double)(A - 1)) : -INFINITY;
}

// st = pi[V] | d  ->  tab
__global__ __launch_bounds__(256) void k_prior_tables(const double* __restrict__ st, int32_t V, int32_t A, double* __restrict__ tab) {
  prior_tables(st, st[V], V, A, tab, (int)threadIdx.x, 256);
}

// mask[b] = the barcode has pairs (K3's record)
__global__ __launch_bounds__(256) void k_prior_mask(const dmx_cell_summary* __restrict__ sum, int32_t B, uint8_t* __restrict__ mask) {
  const int32_t b = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (b < B) mask[b] = sum[b].n_pairs > 0 ? 1 : 0;
}

__device__ inline double wave_sum(double x) {
  for (int s = 1; s < 64; s <<= 1) x += __shfl_xor(x, s);
  return x;
}
__device__ inline double wave_max(double x) {
  for (int s = 1; s < 64; s <<= 1) x = fmax(x, __shfl_xor(x, s));
  return x;
}

// CALL = false: rows[b] = N[V] | homotypic mass | heterotypic mass | log E_b and flag[b] = 0 (included), DMX_PRIOR_MASKED or
// DMX_PRIOR_BAD.  CALL = true: calls[b], which carries the flag (flag[] is not touched).  A flagged barcode gets zeros.
template <bool CALL>
__global__ __launch_bounds__(256) void k_prior_estep(const double* __restrict__ grid, const uint8_t* __restrict__ mask, int32_t B, int32_t V,
                                                     int32_t A, const double* __restrict__ tab, double* __restrict__ rows,
                                                     uint8_t* __restrict__ flag, dmx_prior_call* __restrict__ calls) {
  extern __shared__ double s_pri[];              // colw[V A] | per wavefront: col[V A] | rowv[V] | sv[V]
  const int32_t VA = V * A;
  double* colw = s_pri;                          // log(d / (A - 1)) + log pi_k at slot (k, n >= 1); NaN at the slots n = 0, which are not used
  {
    const double ld = tab[3 * V];
    for (int32_t e = (int32_t)threadIdx.x; e < VA; e += (int32_t)blockDim.x) {
      const int32_t k = e / A;
      colw[e] = (e - k * A) >= 1 ? ld + tab[k] : NAN;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int32_t b = (int32_t)blockIdx.x * (int32_t)(blockDim.x >> 6) + wave;
  if (b >= B) return;
  double* col = s_pri + VA + (size_t)wave * ((size_t)VA + 2 * (size_t)V);
  double* rowv = col + VA;
  double* sv = rowv + V;
  const double* g = grid + (size_t)b * (size_t)V * (size_t)VA;
  const double* lws = tab + V;
  const double* hf = tab + 2 * V;
  double* out = CALL ? nullptr : rows + (size_t)b * ((size_t)V + 3);

  auto write_zero = [&](uint8_t f) {
    if (CALL) {
      if (lane == 0) {
        dmx_prior_call r;
        r.log_e = 0.0; r.p_sng = 0.0; r.p_het = 0.0; r.p_hom = 0.0; r.p_sng1 = 0.0; r.p_sng2 = 0.0; r.p_dbl1 = 0.0;
        r.i_sng1 = -1; r.i_sng2 = -1; r.j_dbl = -1; r.k_dbl = -1; r.n_dbl = -1; r.flag = f;
        calls[b] = r;
      }
    } else {
      for (int32_t v = lane; v < V + 3; v += 64) out[v] = 0.0;
    }
    if (!CALL && lane == 0) flag[b] = f;
  };
  if (mask && !mask[b]) { write_zero(DMX_PRIOR_MASKED); return; }

  // pass 1: the maximum of L + log w over the terms that are not zero; NaN or +inf among the used entries
  double mx = -INFINITY;
  int bad = 0;
  for (int32_t j = lane; j < V; j += 64) {
    const double s = g[(size_t)j * VA], lw = lws[j];
    if (!(s < INFINITY)) bad = 1;
    if (lw > -INFINITY && s > -INFINITY) mx = fmax(mx, s + lw);
  }
  for (int32_t j = 0; j < V; ++j) {
    const double lpj = tab[j];
    const double* row = g + (size_t)j * VA;
    const int32_t dlo = j * A, dhi = dlo + A;    // the diagonal's slots
    for (int32_t e = lane; e < VA; e += 64) {
      const double L = row[e], cw = colw[e];
      if (cw == cw && (e < dlo || e >= dhi)) {
        if (!(L < INFINITY)) bad = 1;
        const double lw = cw + lpj;
        if (lw > -INFINITY && L > -INFINITY) mx = fmax(mx, L + lw);
      }
    }
  }
  mx = wave_max(mx);
  if (__any(bad) || !(mx > -INFINITY)) { write_zero(DMX_PRIOR_BAD); return; }

  // pass 2
  double* xs = col;                              // CALL: the singlet-like terms' logarithms (the column sums are not needed)
  if (!CALL) for (int32_t e = lane; e < VA; e += 64) col[e] = 0.0;
  for (int32_t j = lane; j < V; j += 64) {
    const double s = g[(size_t)j * VA], lw = lws[j];
    const bool on = lw > -INFINITY && s > -INFINITY;
    sv[j] = on ? exp((s + lw) - mx) : 0.0;
    if (CALL) xs[j] = on ? s + lw : -INFINITY;
  }
  double bx = -INFINITY;                         // CALL: this lane's first maximum of the doublet terms, by flat index j V A + e
  int32_t bi = 0x7fffffff;
  for (int32_t j = 0; j < V; ++j) {
    const double lpj = tab[j];
    const double* row = g + (size_t)j * VA;
    const int32_t dlo = j * A, dhi = dlo + A;
    double rp = 0.0;
    for (int32_t e = lane; e < VA; e += 64) {
      const double L = row[e], cw = colw[e];
      const double lw = cw + lpj;
      const bool on = cw == cw && (e < dlo || e >= dhi) && lw > -INFINITY && L > -INFINITY;
      const double x = L + lw;
      const double t = on ? exp(x - mx) : 0.0;
      rp += t;
      if (CALL) {
        if (on && x > bx) { bx = x; bi = j * VA + e; }
      } else {
        col[e] += t;
      }
    }
    rp = wave_sum(rp);
    if (lane == 0) rowv[j] = rp;
  }
  DMX_WAVE_LDS_ORDER();
  double E = 0.0;
  for (int32_t j = 0; j < V; ++j) E += sv[j] + rowv[j];
  double hs = 0.0, hom = 0.0, sng = 0.0;
  for (int32_t j = 0; j < V; ++j) {
    const double r = sv[j] / E, h = r * hf[j];
    hs += rowv[j]; hom += h; sng += r - h;
  }
  const double het = hs / E;
  const double log_e = mx + log(E);
  if (!CALL) {
    for (int32_t k = lane; k < V; k += 64) {
      double cs = 0.0;
      for (int32_t n = 1; n < A; ++n) cs += col[k * A + n];
      const double r = sv[k] / E;
      out[k] = (r + r * hf[k]) + (rowv[k] + cs) / E;
    }
    if (lane == 0) { out[V] = hom; out[V + 1] = het; out[V + 2] = log_e; flag[b] = 0; }
  } else {
    for (int s = 1; s < 64; s <<= 1) {           // the wave's first maximum: the larger term, the lower flat index among equals
      const double ox = __shfl_xor(bx, s);
      const int32_t oi = __shfl_xor(bi, s);
      if (ox > bx || (ox == bx && oi < bi)) { bx = ox; bi = oi; }
    }
    if (lane == 0) {
      int32_t i1 = 0;
      for (int32_t j = 1; j < V; ++j) if (xs[j] > xs[i1]) i1 = j;
      int32_t i2 = i1 == 0 ? 1 : 0;
      for (int32_t j = i2 + 1; j < V; ++j) if (j != i1 && xs[j] > xs[i2]) i2 = j;
      dmx_prior_call r;
      r.log_e = log_e; r.p_sng = sng; r.p_het = het; r.p_hom = hom;
      r.p_sng1 = sv[i1] / E; r.p_sng2 = sv[i2] / E;
      if (bx > -INFINITY) {
        const int32_t j = bi / VA, e = bi - j * VA;
        r.j_dbl = j; r.k_dbl = e / A; r.n_dbl = e - (e / A) * A;
        r.p_dbl1 = exp(bx - mx) / E;
      } else {
        r.j_dbl = -1; r.k_dbl = -1; r.n_dbl = -1; r.p_dbl1 = 0.0;
      }
      r.i_sng1 = i1; r.i_sng2 = i2; r.flag = 0;
      calls[b] = r;
    }
  }
}

// idx = the included barcodes (flag 0) in ascending id, n_in their count.  One workgroup of 1024.
__global__ __launch_bounds__(1024) void k_prior_rank(const uint8_t* __restrict__ flag, int32_t B, int32_t* __restrict__ idx,
                                                     int32_t* __restrict__ n_in) {
  __shared__ int32_t s_w[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t K = (B + 1023) / 1024;           // thread t owns the barcodes t K .. t K + K - 1
  const int32_t b0 = (int32_t)min((int64_t)B, (int64_t)tid * K), b1 = (int32_t)min((int64_t)B, (int64_t)b0 + K);
  int32_t cnt = 0;
  for (int32_t b = b0; b < b1; ++b) cnt += flag[b] == 0;
  int32_t inc = cnt;                             // inclusive scan over the wavefront, then over the 16 wavefronts
  for (int s = 1; s < 64; s <<= 1) {
    const int32_t o = __shfl_up(inc, s);
    if (lane >= s) inc += o;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int32_t off = 0, tot = 0;
  for (int w = 0; w < 16; ++w) { if (w < wave) off += s_w[w]; tot += s_w[w]; }
  int32_t pos = off + inc - cnt;
  for (int32_t b = b0; b < b1; ++b) if (flag[b] == 0) idx[pos++] = b;
  if (tid == 0) *n_in = tot;
}

// part[c] = the rows of the included barcodes of rank 64 c .. 64 c + 63 added in rank order from 0.0, column by column.  Workgroup
// (c, y) stages the chunk's columns 64 y .. 64 y + 63 in LDS with coalesced loads; a lane per column then adds them in rank order.
__global__ __launch_bounds__(256) void k_prior_fold_chunk(const double* __restrict__ rows, const int32_t* __restrict__ idx,
                                                          const int32_t* __restrict__ n_in, int32_t V, double* __restrict__ part) {
  __shared__ double s_t[kPriChunk][64];
  const int32_t n = *n_in, r0 = (int32_t)blockIdx.x * kPriChunk;
  if (r0 >= n) return;                           // (the whole workgroup)
  const int32_t cnt = min(kPriChunk, n - r0), stride = V + 3;
  const int tid = threadIdx.x, cl = tid & 63;
  const int32_t c = (int32_t)blockIdx.y * 64 + cl;
  for (int32_t i = tid >> 6; i < cnt; i += 4) s_t[i][cl] = c < stride ? rows[(size_t)idx[r0 + i] * stride + c] : 0.0;
  __syncthreads();
  if (tid < 64 && c < stride) {
    double s = 0.0;
    for (int32_t i = 0; i < cnt; ++i) s += s_t[i][tid];
    part[(size_t)blockIdx.x * stride + c] = s;
  }
}

// out = N[V] | homotypic mass | heterotypic mass | LL | pi'[V] | d' | B_in: the chunk partials in ascending chunk order from 0.0, then the
// M-step.  apply: st = pi | d takes pi', d' and tab is rebuilt for the next iteration.  One workgroup of 256.
__global__ __launch_bounds__(256) void k_prior_fold(const double* __restrict__ part, const int32_t* __restrict__ n_in, int32_t V, int32_t A,
                                                    int32_t apply, int32_t fix_pi, int32_t fix_d, double* st, double* out, double* tab) {
  __shared__ double s_tot;
  const int tid = threadIdx.x;
  const int32_t n = *n_in, stride = V + 3, nch = (n + kPriChunk - 1) / kPriChunk;
  for (int32_t c = tid; c < stride; c += 256) {
    double s = 0.0;
#pragma unroll 8
    for (int32_t i = 0; i < nch; ++i) s += part[(size_t)i * stride + c];
    out[c] = s;
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int32_t j = 0; j < V; ++j) t += out[j];
    s_tot = t;
    const double dn = (fix_d || n == 0) ? st[V] : fmin((out[V] + out[V + 1]) / (double)n, 1.0);
    out[2 * V + 3] = dn;
    out[2 * V + 4] = (double)n;
  }
  __syncthreads();
  const double tot = s_tot;
  for (int32_t j = tid; j < V; j += 256) out[V + 3 + j] = (fix_pi || !(tot > 0.0)) ? st[j] : out[j] / tot;
  __syncthreads();
  if (apply) {
    for (int32_t j = tid; j < V; j += 256) st[j] = out[V + 3 + j];
    if (tid == 0) st[V] = out[2 * V + 3];
    __syncthreads();
    prior_tables(st, st[V], V, A, tab, tid, 256);
  }
}

}  // namespace dmx_prior
