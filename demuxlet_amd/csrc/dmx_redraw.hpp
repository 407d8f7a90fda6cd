// Model-drawn null pool (dmx_engine_redraw) — included by dmx_engine.hip after dmx_compose.hpp (mix64, kGold).
//
// The staged pileup's layout is kept; every stored read of a used barcode gets a new allele, drawn from dmx_engine_fit's law under the
// barcode's hypothesis: a genotype per hypothesised sample from its gp row, then each read's allele from the drawn component's ALT
// probability at the read's base quality.  include/dmx.h defines the result bit for bit.
//
// k_fit's skeleton: the phred tables in LDS, one wavefront per used barcode, lane l takes pairs l, l + 64, ... of the barcode, 64 pair
// headers per trip, read offsets by the DPP scan.  A lane walks its pair's reads serially: one byte load, one hash, five FP64 operations
// and a division, one byte store.  The host has copied the whole read array to the output first, so unused barcodes, pairs without
// stored reads, skipped pairs and reads whose probability is not in [0, 1] need no store.  No atomics and nothing from another
// barcode: the four counts of a barcode are added over its lanes in lane order by lane 0.
#pragma once

namespace dmx_rdw {

constexpr int kWaves = 4;                        // wavefronts (= used barcodes) per workgroup; they share the phred tables

struct Ctx {
  PileupView pv; int nrd_width;                  // the source
  const double* tabs;                            // mat[128] | err / 3 [128] | ...
  const float* g; int32_t V;
  const int32_t* idx; int32_t n_idx;             // the used barcodes
  const int32_t* hyp; const double* alpha; const double* rho; const double* amb;
  uint64_t seed, geno_seed; int64_t index_base;
  int32_t donor_draw;                            // DMX_REDRAW_DONOR
  int32_t B;
  uint8_t* o_reads;                              // [pv.R], a copy of pv.reads when the kernel starts
  int8_t* o_geno;                                // [pairs][2], -1 when the kernel starts
  int32_t* cnt;                                  // [4][B]: pairs drawn | pairs skipped | reads drawn | reads kept
};

// a gp row that can be drawn from: no negative or non-finite entry, not all zero
__device__ __forceinline__ bool row_ok(float w0, float w1, float w2) {
  const bool fin = fabsf(w0) < INFINITY && fabsf(w1) < INFINITY && fabsf(w2) < INFINITY;
  return fin && w0 >= 0.f && w1 >= 0.f && w2 >= 0.f && (w0 != 0.f || w1 != 0.f || w2 != 0.f);
}

// The genotype of a row at the 32-bit uniform ug.  x < s strictly (ug 2^-32 <= 1 - 2^-32, and s is a normal float64), so x never
// reaches the last cumulative sum; a zero weight makes two neighbouring cumulative sums equal, and no x lies in an empty interval.
__device__ __forceinline__ int draw_genotype(float f0, float f1, float f2, uint32_t ug) {
  const double w0 = (double)f0, w1 = (double)f1, w2 = (double)f2;
  const double c01 = w0 + w1;
  const double s = c01 + w2;
  const double x = ((double)ug * 0x1p-32) * s;
  return x < w0 ? 0 : x < c01 ? 1 : 2;
}

__device__ __forceinline__ uint32_t geno_uniform(uint64_t key, int32_t snp) {
  return (uint32_t)(dmx_cmp::mix64(key + ((uint64_t)(uint32_t)snp << 32)) >> 32);
}

__global__ __launch_bounds__(64 * kWaves) void k_redraw(Ctx c) {
  __shared__ double s_me[128][2];                // by base quality: {mat, err / 3}
  __shared__ int32_t s_cnt[kWaves][64][4];
  for (int i = threadIdx.x; i < 128; i += 64 * kWaves) { s_me[i][0] = c.tabs[i]; s_me[i][1] = c.tabs[128 + i]; }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int32_t unit = (int32_t)blockIdx.x * kWaves + wave;
  if (unit >= c.n_idx) return;
  const int32_t cell = __builtin_amdgcn_readfirstlane(c.idx[unit]);
  const int32_t v1 = __builtin_amdgcn_readfirstlane(c.hyp[2 * (size_t)cell]);
  const int32_t v2 = __builtin_amdgcn_readfirstlane(c.hyp[2 * (size_t)cell + 1]);
  const bool dbl = v2 >= 0;
  const double rh = c.rho[cell], om = 1.0 - rh, al = c.alpha[cell];
  const uint64_t id = (uint64_t)c.index_base + (uint64_t)(uint32_t)cell;
  const uint64_t key_r = dmx_cmp::mix64(c.seed + dmx_cmp::kGold * (4ull * id + 1ull));
  const uint64_t key_1 = c.donor_draw ? dmx_cmp::mix64(c.geno_seed + dmx_cmp::kGold * (4ull * (uint64_t)(uint32_t)v1 + 2ull))
                                      : dmx_cmp::mix64(c.seed + dmx_cmp::kGold * (4ull * id + 2ull));
  const uint64_t key_2 = c.donor_draw ? dmx_cmp::mix64(c.geno_seed + dmx_cmp::kGold * (4ull * (uint64_t)(uint32_t)(dbl ? v2 : 0) + 2ull))
                                      : dmx_cmp::mix64(c.seed + dmx_cmp::kGold * (4ull * id + 3ull));
  int32_t n_drawn = 0, n_skip = 0, r_drawn = 0, r_kept = 0;
  const int64_t p_beg = c.pv.cell_pair_off[cell], p_end = c.pv.cell_pair_off[cell + 1];
  int64_t rd_base = c.pv.cell_read_off[cell];
  for (int64_t p0 = p_beg; p0 < p_end; p0 += 64) {
    const int64_t p = p0 + lane;
    const bool in = p < p_end;
    const uint32_t n = in ? load_nrd(c.pv.pair_nrd, p, c.nrd_width) : 0u;
    const uint32_t incl = seg_scan_incl<64>(n);
    const int64_t off = rd_base + (int64_t)(incl - n);
    rd_base += (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (n > 0u) {
      const int32_t snp = c.pv.pair_snp ? c.pv.pair_snp[p] : (int32_t)(p - p_beg);
      const float* gs = c.g + (size_t)snp * c.V * 3;
      const float* r1 = gs + (size_t)v1 * 3;
      const float x0 = r1[0], x1 = r1[1], x2 = r1[2];
      bool ok = row_ok(x0, x1, x2);
      float y0 = 0.f, y1 = 0.f, y2 = 0.f;
      if (dbl) {
        const float* r2 = gs + (size_t)v2 * 3;
        y0 = r2[0]; y1 = r2[1]; y2 = r2[2];
        ok = ok && row_ok(y0, y1, y2);
      }
      if (!ok) {
        n_skip += 1;
      } else {
        const int l = draw_genotype(x0, x1, x2, geno_uniform(key_1, snp));
        int m = -1;
        double cm = 0.5 * l;
        if (dbl) {
          m = draw_genotype(y0, y1, y2, geno_uniform(key_2, snp));
          cm = 0.5 * l + (m - l) * 0.5 * al;
        }
        c.o_geno[2 * p] = (int8_t)l; c.o_geno[2 * p + 1] = (int8_t)m;
        const double ra = rh * c.amb[snp];
        const double pc = om * cm + ra, q1 = 1.0 - pc;
        const uint64_t key_p = key_r + ((uint64_t)(uint32_t)snp << 32);   // + r below: (snp << 32 | r), r < 2^32
        n_drawn += 1;
        for (uint32_t r = 0; r < n; ++r) {
          const int64_t at = off + (int64_t)r;
          if (at >= c.pv.R) break;                 // (never for a pileup that passed dmx_engine_set_pileup)
          const uint32_t bq = c.pv.reads[at] & 127u;
          const double mat = s_me[bq][0], e3 = s_me[bq][1];
          const double num = e3 * q1 + mat * pc;
          const double den = mat + e3;
          const double q = num / den;
          if (q >= 0.0 && q <= 1.0) {
            const uint64_t thr = (uint64_t)(q * 4294967296.0);
            const uint64_t u = dmx_cmp::mix64(key_p + (uint64_t)r) >> 32;
            c.o_reads[at] = (uint8_t)(bq | (u < thr ? 128u : 0u));
            r_drawn += 1;
          } else {
            r_kept += 1;
          }
        }
      }
    }
  }
  s_cnt[wave][lane][0] = n_drawn; s_cnt[wave][lane][1] = n_skip; s_cnt[wave][lane][2] = r_drawn; s_cnt[wave][lane][3] = r_kept;
  DMX_WAVE_LDS_ORDER();
  if (lane == 0) {
    int32_t k0 = 0, k1 = 0, k2 = 0, k3 = 0;
    for (int l = 0; l < 64; ++l) { k0 += s_cnt[wave][l][0]; k1 += s_cnt[wave][l][1]; k2 += s_cnt[wave][l][2]; k3 += s_cnt[wave][l][3]; }
    c.cnt[cell] = k0; c.cnt[(size_t)c.B + cell] = k1; c.cnt[2 * (size_t)c.B + cell] = k2; c.cnt[3 * (size_t)c.B + cell] = k3;
  }
}

}  // namespace dmx_rdw
