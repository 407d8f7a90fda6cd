// Block-resolved likelihoods (dmx_engine_block_llk).  Included into dmx_engine.hip after the anchored search,
// whose helpers and tile shape it shares.
//
// k_block_col is k_anchor_col with a segmented accumulator: one wavefront per (barcode, slab of 64 entries), tiles of
// TP = min(32, 64 / A_pad) covered pairs, phase 1 on lane (pair, alpha) exactly as anchor_body (pair_values_open / rcp_refined / div_by,
// the nine finished values and — in slab 0 — the pair's llks00 term to LDS), phase 2 on lane = entry walking the tile's pairs in
// ascending order.  The entries of a barcode are the V singlet entries (j, 0, 0) and then its E extra entries (j, k, n); lane < A of
// slab 0 also carries llks00[lane], and lane 0 of slab 0 the pair count.
// block[] is non-decreasing and a barcode's pairs are SNP-sorted, so the block of pair ti is the same for the whole wavefront and
// never returns: a lane keeps ONE live accumulator, stores it when the block changes and restarts at +0.  A value is therefore one
// serial sum from +0 over the block's pairs in stored order, with the operations of the STRICT grid's entry; blocks the barcode does
// not cover are never written and keep the zeros the host put there.
// No argument-class test and no fix-up pass: the host refuses a matrix that k_check_geno did not pass, and it has checked block[] and
// extra[] (both are the call's own device copies), so every index below is in range.
#pragma once

namespace dmx_blk {

constexpr int kWaves = kAncWaves, kTP = kAncTP, kMaxExtra = 8;
constexpr uint32_t kNone = kAncNone;

__global__ __launch_bounds__(64 * kWaves) void k_block_col(PileupView pv, int nrd_width, const float* __restrict__ g, const double* __restrict__ gp0,
                                                         const double* __restrict__ tabs, const double* __restrict__ alpha, int32_t V, int32_t A,
                                                         int32_t A_pad, int32_t TP, const int32_t* __restrict__ block, int32_t G,
                                                         const int32_t* __restrict__ extra, int32_t E, int32_t n_slab, int64_t n_units,
                                                         double* __restrict__ col, double* __restrict__ l00, double* __restrict__ ext,
                                                         int32_t* __restrict__ n_snp) {
  __shared__ double s_tab[kTab2];
  __shared__ double s_pGs[kWaves][64 * 9];
  __shared__ double s_t00s[kWaves][64];
  __shared__ int32_t s_snps[kWaves][kTP];
  __shared__ int32_t s_blks[kWaves][kTP];
  __shared__ uint32_t s_cnts[kWaves][kTP];
  __shared__ int64_t s_offs[kWaves][kTP];
  stage_k2_tables(s_tab, tabs, threadIdx.x, 64 * kWaves);
  __syncthreads();
  const double* s_log = s_tab + kLut2;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t unit = (int64_t)blockIdx.x * kWaves + wave;
  if (unit >= n_units) return;
  const int32_t cell = (int32_t)(unit / n_slab), slab = (int32_t)(unit % n_slab);
  double* s_pG = s_pGs[wave]; double* s_t00 = s_t00s[wave];
  int32_t* s_snp = s_snps[wave]; int32_t* s_blk = s_blks[wave]; uint32_t* s_cnt = s_cnts[wave]; int64_t* s_off = s_offs[wave];

  // this lane's entry: code = (j << 20) | (k << 8) | n, and where block g's sum goes: dst[g * stride]
  uint32_t code = kNone;
  double* dst = nullptr;
  int64_t stride = 0;
  {
    const int64_t en = (int64_t)slab * 64 + lane;
    if (en < V) {
      code = (uint32_t)en << 20;
      dst = col + (int64_t)cell * G * V + en; stride = V;
    } else if (en < (int64_t)V + E) {
      const int32_t slot = (int32_t)(en - V);
      const int32_t* x = extra + ((int64_t)cell * E + slot) * 3;
      if (x[0] >= 0) {
        code = ((uint32_t)x[0] << 20) | ((uint32_t)x[1] << 8) | (uint32_t)x[2];
        dst = ext + (int64_t)cell * G * E + slot; stride = E;
      }
    }
  }
  const bool do00 = slab == 0;
  double acc = 0.0, acc00 = 0.0;
  int32_t cur = -1, n_in = 0;                       // the block being summed (wave-uniform) and its pairs so far
  auto flush = [&]() {
    if (dst) dst[(int64_t)cur * stride] = acc;
    if (do00 && lane < A) l00[((int64_t)cell * G + cur) * A + lane] = acc00;
    if (do00 && lane == 0) n_snp[(int64_t)cell * G + cur] = n_in;
  };

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
    load_tile_headers<kTP>(pv, nrd_width, p_beg, tbase, tp, lane, rd_base, s_cnt, s_off, s_snp);
    DMX_WAVE_LDS_ORDER();
    rd_base = s_off[tp - 1] + (int64_t)s_cnt[tp - 1];
    if (lane < tp) s_blk[lane] = block[s_snp[lane]];
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
      const int32_t blk = __builtin_amdgcn_readfirstlane(s_blk[ti]);
      if (blk != cur) {
        if (cur >= 0) flush();
        cur = blk; acc = 0.0; acc00 = 0.0; n_in = 0;
      }
      ++n_in;
      if (code != kNone) {
        const int32_t snp = s_snp[ti];
        const float* __restrict__ grow = g + (size_t)snp * V * 3;
        const int32_t j = (code >> 20) & 0xFFF, k = (code >> 8) & 0xFFF, n = code & 0xFF;
        const double a[3] = {(double)grow[j * 3], (double)grow[j * 3 + 1], (double)grow[j * 3 + 2]};
        const double b[3] = {(double)grow[k * 3], (double)grow[k * 3 + 1], (double)grow[k * 3 + 2]};
        const double* P = &s_pG[(ti * A + n) * 9];
        double sum = 0.0;                                                          // :674
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int m = 0; m < 3; ++m) sum += ((a[l] * b[m]) * P[l * 3 + m]);       // :553 then :677-679, l-major
        acc += dmx_log2_fast(sum, s_log);                                          // :683
      }
      if (do00 && lane < A) acc00 += s_t00[ti * A + lane];                         // :709
    }
    DMX_WAVE_LDS_ORDER();
  }
  if (cur >= 0) flush();
}

}  // namespace dmx_blk
