// Joint genotype tables (dmx_engine_geno_compare) — included by dmx_engine.hip at its end.
//
// T[a][b][x][y] = sum over the SNPs of wa_i[a][x] * rb_i[b][y], one ascending fma chain per entry; include/dmx.h defines the bits.
//
// k_kin_rows turns a gp matrix [S][V][3] float32 into the [S][V][4] float64 image (p0, p1, p2, m), times c_i on the A side, and counts
// the invalid rows per column with integer atomics (a count does not depend on the order of its increments).
//
// k_kin_tile is the contraction.  A workgroup of 256 threads, 16 x 16, owns TA x TB = 16 BA x 16 BB column pairs; thread (ty, tx) keeps the
// BA x BB pairs (ty + 16 u, tx + 16 v) x 16 entries in registers.  The SNPs are walked in ascending order, kChunk (a template argument) at a time, through two
// LDS buffers: the 16-byte pieces of chunk k + 1 are loaded from global memory into registers before chunk k is multiplied and written
// to the other buffer after it, one barrier per chunk.  In LDS a SNP's vectors lie as [half][column] double2 (half 0 = (p0, p1),
// half 1 = (p2, m)): the 16 lanes that differ in tx read 16 consecutive 16-byte slots, the lanes that differ in ty read one slot each
// (a broadcast within the other 16), so no ds_read_b128 has a bank conflict; a thread's staging write goes to slot threadIdx.x + 256 k.
// Columns past VA / VB are zero-filled pieces: a zero operand only ever feeds the entries of a pair that is not written.  The SNP
// tail is not padded: the last chunk's loop runs to the true S.  No atomics, no partial sums, nothing from another workgroup.
#pragma once

namespace dmx_kin {

constexpr int kThreads = 256;                    // 16 x 16
constexpr int kChunkNarrow = 24, kChunkWide = 8;   // SNPs staged per trip: the narrow block has 16 fma per SNP to hide a global load behind
constexpr int kWideTiles = 256;                  // the 2 x 2 block is used when its tiling gives at least this many workgroups

__global__ __launch_bounds__(256) void k_kin_rows(const float* __restrict__ g, int64_t n, int32_t V, const double* __restrict__ c,
                                                  double* __restrict__ img, int32_t* __restrict__ n_invalid) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += step) {
    const float f0 = g[3 * t], f1 = g[3 * t + 1], f2 = g[3 * t + 2];
    const double g0 = (double)f0, g1 = (double)f1, g2 = (double)f2;
    const double s = (g0 + g1) + g2;
    const bool ok = s > 0.0 && s < INFINITY && f0 >= 0.f && f1 >= 0.f && f2 >= 0.f;   // (a NaN fails s > 0 or its own >=)
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, m = 0.0;
    if (ok) { p0 = g0 / s; p1 = g1 / s; p2 = g2 / s; m = 1.0; }
    if (c) {
      const double w = c[t / V];
      p0 = w * p0; p1 = w * p1; p2 = w * p2; m = w * m;
    }
    double2* o = (double2*)(img + 4 * t);
    o[0] = make_double2(p0, p1); o[1] = make_double2(p2, m);
    if (!ok) atomicAdd(&n_invalid[t % V], 1);
  }
}

// the 16-byte piece q of a chunk's side: [SNP][half][column of the tile]
template <int TC>
__device__ __forceinline__ double2 load_piece(const double* __restrict__ img, int32_t S, int32_t V, int32_t i0, int32_t c0, int q) {
  const int64_t i = (int64_t)i0 + q / (2 * TC);
  const int32_t col = c0 + q % TC;
  const int half = (q / TC) & 1;
  if (i >= S || col >= V) return make_double2(0.0, 0.0);
  return *(const double2*)(img + ((size_t)i * (size_t)V + (size_t)col) * 4 + 2 * half);
}

template <int BA, int BB>
__device__ __forceinline__ void fma_snp(const double2* __restrict__ pa, const double2* __restrict__ pb, int ty, int tx,
                                        double (&acc)[BA][BB][4][4]) {
  constexpr int TA = 16 * BA, TB = 16 * BB;
  double a[BA][4], b[BB][4];
#pragma unroll
  for (int u = 0; u < BA; ++u) {
    const double2 lo = pa[ty + 16 * u], hi = pa[TA + ty + 16 * u];
    a[u][0] = lo.x; a[u][1] = lo.y; a[u][2] = hi.x; a[u][3] = hi.y;
  }
#pragma unroll
  for (int v = 0; v < BB; ++v) {
    const double2 lo = pb[tx + 16 * v], hi = pb[TB + tx + 16 * v];
    b[v][0] = lo.x; b[v][1] = lo.y; b[v][2] = hi.x; b[v][3] = hi.y;
  }
#pragma unroll
  for (int u = 0; u < BA; ++u)
#pragma unroll
    for (int v = 0; v < BB; ++v)
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[u][v][x][y] = __builtin_fma(a[u][x], b[v][y], acc[u][v][x][y]);
}

template <int BA, int BB, int kChunk>
__global__ __launch_bounds__(kThreads, 2) void k_kin_tile(const double* __restrict__ ia, const double* __restrict__ ib, int32_t S, int32_t VA,
                                                       int32_t VB, double* __restrict__ T) {
  constexpr int TA = 16 * BA, TB = 16 * BB;
  constexpr int PA = kChunk * 2 * TA, PB = kChunk * 2 * TB;          // 16-byte pieces per chunk and side
  constexpr int NA = PA / kThreads, NB = PB / kThreads;              // ... per thread
  constexpr int kUnroll = BA * BB == 1 ? kChunk : 1;                 // (the wide block: 128 accumulator VGPRs; two waves per SIMD leave it 256 in all)
  static_assert(PA % kThreads == 0 && PB % kThreads == 0, "a thread stages whole pieces of one side");
  extern __shared__ __attribute__((aligned(16))) char s_kin[];      // two buffers of PA + PB pieces; no static LDS in front of it
  double2* const s_buf = (double2*)s_kin;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int32_t a0 = (int32_t)blockIdx.y * TA, b0 = (int32_t)blockIdx.x * TB;
  double acc[BA][BB][4][4];
#pragma unroll
  for (int u = 0; u < BA; ++u)
#pragma unroll
    for (int v = 0; v < BB; ++v)
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[u][v][x][y] = 0.0;
  const int32_t n_chunks = (int32_t)(((int64_t)S + kChunk - 1) / kChunk);
  double2 ra[NA], rb[NB];
  if (n_chunks > 0) {
#pragma unroll
    for (int k = 0; k < NA; ++k) s_buf[tid + kThreads * k] = load_piece<TA>(ia, S, VA, 0, a0, tid + kThreads * k);
#pragma unroll
    for (int k = 0; k < NB; ++k) s_buf[PA + tid + kThreads * k] = load_piece<TB>(ib, S, VB, 0, b0, tid + kThreads * k);
    __syncthreads();
  }
  for (int32_t ch = 0; ch < n_chunks; ++ch) {
    const int32_t i0 = ch * kChunk;               // (i0 < S, and i0 + kChunk < S where a next chunk exists)
    const bool more = ch + 1 < n_chunks;
    if (more) {
#pragma unroll
      for (int k = 0; k < NA; ++k) ra[k] = load_piece<TA>(ia, S, VA, i0 + kChunk, a0, tid + kThreads * k);
#pragma unroll
      for (int k = 0; k < NB; ++k) rb[k] = load_piece<TB>(ib, S, VB, i0 + kChunk, b0, tid + kThreads * k);
    }
    const double2* cur = s_buf + (size_t)(ch & 1) * (PA + PB);
    const int n_here = S - i0 < kChunk ? S - i0 : kChunk;   // the tail runs to the true S: no padding steps
    if (kUnroll > 1 && n_here == kChunk) {
#pragma unroll
      for (int s = 0; s < kChunk; ++s) fma_snp<BA, BB>(cur + s * 2 * TA, cur + PA + s * 2 * TB, ty, tx, acc);
    } else {
#pragma unroll 1
      for (int s = 0; s < n_here; ++s) fma_snp<BA, BB>(cur + s * 2 * TA, cur + PA + s * 2 * TB, ty, tx, acc);
    }
    if (more) {
      double2* nxt = s_buf + (size_t)((ch + 1) & 1) * (PA + PB);   // last read in trip ch - 1, before that trip's barrier
#pragma unroll
      for (int k = 0; k < NA; ++k) nxt[tid + kThreads * k] = ra[k];
#pragma unroll
      for (int k = 0; k < NB; ++k) nxt[PA + tid + kThreads * k] = rb[k];
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < BA; ++u)
#pragma unroll
    for (int v = 0; v < BB; ++v) {
      const int32_t a = a0 + ty + 16 * u, b = b0 + tx + 16 * v;
      if (a < VA && b < VB) {
        double2* o = (double2*)(T + ((size_t)a * (size_t)VB + (size_t)b) * 16);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          o[2 * x] = make_double2(acc[u][v][x][0], acc[u][v][x][1]);
          o[2 * x + 1] = make_double2(acc[u][v][x][2], acc[u][v][x][3]);
        }
      }
    }
}

}  // namespace dmx_kin
