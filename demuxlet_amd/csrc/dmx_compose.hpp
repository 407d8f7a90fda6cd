// Pileup composer (dmx_engine_compose) — included by dmx_engine.hip.
//
// New barcodes from the reads of one or two barcodes of the staged pileup, every read kept or dropped by a hash of (output id, slot, SNP id,
// index in the pair): in-silico doublets and thinned barcodes.  Integers only; include/dmx.h defines the result bit for bit.
//
// count -> scan -> fill.  Count and fill are ONE kernel template: a wavefront per output barcode merges its two parents' sorted pair lists
// in rounds.  A round loads the next (up to) 64 pairs of each parent, one pair per lane, hashes their reads, and settles every pair whose
// SNP id is <= bound = the smaller of the two tiles' last SNP ids (the last id of the only tile when one parent is used up): for those, all
// pairs of the other parent with a smaller id are either settled already or in its current tile, so the pair's place in the output is
//     pairs written so far + surviving pairs before it in its own tile + surviving pairs of smaller id in the other tile
//     - SNPs before it that survive in both tiles (one output pair),
// from two ballots, a binary search of the other tile's ids in LDS and popcounts; read offsets likewise from the tiles' prefix sums of kept reads.
// The tile whose last id is the bound is used up, so a round always advances; a tile settled in part is loaded again from where it stopped
// (its reads are hashed again: at most twice the work).  The count pass runs the same rounds and writes three numbers per barcode; since
// both passes are the same code, the fill pass writes exactly what the count pass promised — and checks every index against its
// barcode's range anyway.  No atomics, no cross-wavefront step: the bits cannot depend on scheduling.
#pragma once

namespace dmx_cmp {

constexpr int kWaves = 4;                        // wavefronts (= output barcodes) per workgroup
constexpr uint64_t kGold = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kKeepAll = 1ull << 32;
constexpr int32_t kMaxOut = 1 << 24;             // output barcodes of one call (dmx_engine_compose checks it): what k_compose_scan's one workgroup is meant for

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Ctx {
  PileupView pv; int nrd_width;                  // the source
  int32_t n_out; int64_t index_base; uint64_t seed;
  const int32_t* parent; const uint64_t* keep;   // [n_out][2]
  int64_t* cnt_pairs; int64_t* cnt_reads; uint32_t* cnt_max;   // count pass out: union pairs, kept reads, largest merged count of a pair
  const int64_t* o_pair_off; const int64_t* o_read_off;        // fill pass in (the scans)
  int32_t* o_snp; void* o_nrd; int o_width; uint8_t* o_reads;  // fill pass out
};

// one parent pair in one lane
struct Elem {
  int32_t snp;                                   // INT32_MAX past the parent's end (SNP ids are < 2^31 - 1), so that a tile is sorted as a whole
  uint32_t n, kept;                              // stored reads, kept reads
  uint64_t km;                                   // bit r: read r < 64 is kept
  bool valid, surv;
};

__device__ __forceinline__ bool read_kept(uint64_t key, uint64_t keep, int32_t snp, uint32_t r) {
  return (mix64(key + (((uint64_t)(uint32_t)snp << 32) | (uint64_t)r)) >> 32) < keep;
}

__device__ __forceinline__ Elem load_elem(const PileupView& pv, int w, int64_t p0, int64_t idx, int64_t np, uint64_t key, uint64_t keep) {
  Elem e;
  e.valid = idx < np; e.snp = 0x7fffffff; e.n = 0u; e.kept = 0u; e.km = 0ull; e.surv = false;
  if (e.valid) {
    const int64_t p = p0 + idx;
    e.n = load_nrd(pv.pair_nrd, p, w);
    e.snp = pv.pair_snp ? pv.pair_snp[p] : (int32_t)idx;
    if (keep >= kKeepAll) {                      // every 32-bit hash is below 2^32
      e.kept = e.n; e.km = e.n >= 64u ? ~0ull : ((1ull << e.n) - 1ull); e.surv = true;
    } else if (e.n == 0u) {
      e.surv = read_kept(key, keep, e.snp, 0u);  // a pair without stored reads: as if it held one read of index 0
    } else {
      for (uint32_t r = 0; r < e.n; ++r)
        if (read_kept(key, keep, e.snp, r)) { ++e.kept; if (r < 64u) e.km |= 1ull << r; }
      e.surv = e.kept > 0u;
    }
  }
  return e;
}

__device__ __forceinline__ uint64_t lanes_below(int x) { return x >= 64 ? ~0ull : ((1ull << x) - 1ull); }

// the number of entries of the sorted tile s[0..64) that are < x
__device__ __forceinline__ int tile_lower_bound(const int32_t* s, int32_t x) {
  int j = 0;
#pragma unroll
  for (int step = 32; step > 0; step >>= 1) if (s[j + step - 1] < x) j += step;
  if (s[j] < x) ++j;
  return j;
}

__device__ __forceinline__ void store_nrd(void* base, int64_t p, int width, uint32_t v) {
  if (width == 1) ((uint8_t*)base)[p] = (uint8_t)v;
  else if (width == 2) ((uint16_t*)base)[p] = (uint16_t)v;
  else ((uint32_t*)base)[p] = v;
}

// the kept reads of one parent pair -> the output's read bytes from dst on (never at or past end)
__device__ __forceinline__ void copy_kept(const Ctx& c, const Elem& e, uint64_t key, uint64_t keep, int64_t src, int64_t dst, int64_t end) {
  const bool all = keep >= kKeepAll;
  for (uint32_t r = 0; r < e.n; ++r) {
    const bool k = all || (r < 64u ? ((e.km >> r) & 1ull) != 0ull : read_kept(key, keep, e.snp, r));
    if (k && src + r < c.pv.R) {
      if (dst < end) c.o_reads[dst] = c.pv.reads[src + r];
      ++dst;
    }
  }
}

template <bool FILL>
__global__ __launch_bounds__(64 * kWaves) void k_compose(Ctx c) {
  __shared__ int32_t s_snp[kWaves][2][64];
  __shared__ uint32_t s_pk[kWaves][2][65];       // exclusive prefix sums of the tiles' kept reads; [64] = the tile's total
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int32_t o = (int32_t)blockIdx.x * kWaves + wave;
  if (o >= c.n_out) return;
  const PileupView& pv = c.pv;
  const int32_t c0 = c.parent[2 * (size_t)o], c1 = c.parent[2 * (size_t)o + 1];
  const uint64_t keep0 = c.keep[2 * (size_t)o], keep1 = c.keep[2 * (size_t)o + 1];
  const uint64_t id = (uint64_t)c.index_base + (uint64_t)o;
  const uint64_t key0 = mix64(c.seed + kGold * (2ull * id + 1ull)), key1 = mix64(c.seed + kGold * (2ull * id + 2ull));
  const int64_t pa0 = pv.cell_pair_off[c0], na = pv.cell_pair_off[c0 + 1] - pa0;
  const int64_t pb0 = c1 >= 0 ? pv.cell_pair_off[c1] : 0, nb = c1 >= 0 ? pv.cell_pair_off[c1 + 1] - pb0 : 0;
  int64_t ra = pv.cell_read_off[c0], rb = c1 >= 0 ? pv.cell_read_off[c1] : 0;      // source read offsets of the tiles' first pairs
  int64_t ia = 0, ib = 0;
  int64_t out_p = FILL ? c.o_pair_off[o] : 0, out_r = FILL ? c.o_read_off[o] : 0;
  const int64_t end_p = FILL ? c.o_pair_off[o + 1] : 0, end_r = FILL ? c.o_read_off[o + 1] : 0;
  uint32_t mx = 0u;
  int32_t* sa = s_snp[wave][0]; int32_t* sb = s_snp[wave][1];
  uint32_t* pka = s_pk[wave][0]; uint32_t* pkb = s_pk[wave][1];
  while (ia < na || ib < nb) {
    const Elem a = load_elem(pv, c.nrd_width, pa0, ia + lane, na, key0, keep0);
    const Elem b = load_elem(pv, c.nrd_width, pb0, ib + lane, nb, key1, keep1);
    const int va = (int)min<int64_t>(64, na - ia), vb = (int)min<int64_t>(64, nb - ib);
    const uint32_t an = seg_scan_incl<64>(a.n), ak = seg_scan_incl<64>(a.kept);
    const uint32_t bn = seg_scan_incl<64>(b.n), bk = seg_scan_incl<64>(b.kept);
    const uint64_t ma = __ballot(a.surv), mb = __ballot(b.surv);
    sa[lane] = a.snp; sb[lane] = b.snp;
    pka[lane] = ak - a.kept; pkb[lane] = bk - b.kept;
    if (lane == 63) { pka[64] = ak; pkb[64] = bk; }
    DMX_WAVE_LDS_ORDER();
    int32_t bound;
    if (va == 0) bound = sb[vb - 1];
    else if (vb == 0) bound = sa[va - 1];
    else bound = min(sa[va - 1], sb[vb - 1]);
    const bool fin_a = a.valid && a.snp <= bound, fin_b = b.valid && b.snp <= bound;
    const uint64_t fa = __ballot(fin_a), fb = __ballot(fin_b);
    const int ca = __popcll(fa), cb = __popcll(fb);                     // settled pairs: a prefix of each tile
    // slot 0's pairs
    const bool wa = fin_a && a.surv;
    int j = 0; bool dup_a = false;
    if (wa) {
      j = tile_lower_bound(sb, a.snp);
      dup_a = j < 64 && sb[j] == a.snp && ((mb >> j) & 1ull) != 0ull;
    }
    const uint64_t dm = __ballot(dup_a);                                 // slot-0 lanes whose SNP survives in slot 1 too
    if (wa) {
      const uint32_t merged = a.kept + (dup_a ? pkb[j + 1] - pkb[j] : 0u);
      mx = max(mx, merged);
      if (FILL) {
        const int64_t pos = out_p + __popcll(ma & lanes_below(lane)) + __popcll(mb & lanes_below(j)) - __popcll(dm & lanes_below(lane));
        if (pos < end_p) { c.o_snp[pos] = a.snp; store_nrd(c.o_nrd, pos, c.o_width, merged); }
        copy_kept(c, a, key0, keep0, ra + (int64_t)(an - a.n), out_r + (int64_t)(ak - a.kept) + (int64_t)pkb[j], end_r);
      }
    }
    // slot 1's pairs: one of a SNP that slot 0 keeps too adds its reads behind slot 0's and no pair of its own
    if (fin_b && b.surv) {
      const int i = tile_lower_bound(sa, b.snp);
      const bool same = i < 64 && sa[i] == b.snp;
      const bool dup_b = same && ((ma >> i) & 1ull) != 0ull;
      if (!dup_b) mx = max(mx, b.kept);
      if (FILL) {
        if (!dup_b) {
          const int64_t pos = out_p + __popcll(mb & lanes_below(lane)) + __popcll(ma & lanes_below(i)) - __popcll(dm & lanes_below(i));
          if (pos < end_p) { c.o_snp[pos] = b.snp; store_nrd(c.o_nrd, pos, c.o_width, b.kept); }
        }
        copy_kept(c, b, key1, keep1, rb + (int64_t)(bn - b.n), out_r + (int64_t)(bk - b.kept) + (int64_t)pka[i + (same ? 1 : 0)], end_r);
      }
    }
    out_p += __popcll(ma & fa) + __popcll(mb & fb) - __popcll(dm);
    out_r += (int64_t)pka[ca] + (int64_t)pkb[cb];
    ra += (int64_t)(ca > 0 ? (uint32_t)__shfl((int)an, ca - 1) : 0u);
    rb += (int64_t)(cb > 0 ? (uint32_t)__shfl((int)bn, cb - 1) : 0u);
    ia += ca; ib += cb;
    DMX_WAVE_LDS_ORDER();                        // the next round's tiles overwrite these
  }
  if (!FILL) {
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
    if (lane == 0) { c.cnt_pairs[o] = out_p; c.cnt_reads[o] = out_r; c.cnt_max[o] = mx; }
  }
}

// exclusive scans of the per-barcode pair and read counts (int64) and the largest merged count; totals[0..3) = pairs, reads, largest merged
// count.  One workgroup: each thread sums its n / 1024 counts, thread 0 scans the 1 024 sums, each thread writes its offsets — 0.1 ms for
// 20 000 barcodes, serial work that grows with n / 1024.  n <= kMaxOut = 2^24 (checked on the host), so t * per <= n + 1 023 fits int32.
__global__ __launch_bounds__(1024) void k_compose_scan(const int64_t* __restrict__ np, const int64_t* __restrict__ nr, const uint32_t* __restrict__ nm,
                                                       int32_t n, int64_t* __restrict__ poff, int64_t* __restrict__ roff, int64_t* __restrict__ totals) {
  __shared__ long long s_a[1024], s_b[1024];
  __shared__ uint32_t s_m[1024];
  const int t = threadIdx.x;
  const int32_t per = (n + 1023) / 1024, lo = min(n, t * per), hi = min(n, lo + per);
  long long a = 0, b = 0; uint32_t m = 0u;
  for (int32_t i = lo; i < hi; ++i) { a += np[i]; b += nr[i]; m = max(m, nm[i]); }
  s_a[t] = a; s_b[t] = b; s_m[t] = m;
  __syncthreads();
  if (t == 0) {
    long long ra = 0, rb = 0; uint32_t rm = 0u;
    for (int i = 0; i < 1024; ++i) { const long long xa = s_a[i], xb = s_b[i]; s_a[i] = ra; s_b[i] = rb; ra += xa; rb += xb; rm = max(rm, s_m[i]); }
    poff[n] = ra; roff[n] = rb;
    totals[0] = ra; totals[1] = rb; totals[2] = (long long)rm;
  }
  __syncthreads();
  a = s_a[t]; b = s_b[t];
  for (int32_t i = lo; i < hi; ++i) { poff[i] = a; roff[i] = b; a += np[i]; b += nr[i]; }
}

}  // namespace dmx_cmp
