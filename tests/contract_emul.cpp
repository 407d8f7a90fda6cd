// Test helper (CPU): the feature passes' contracts of include/dmx.h restated as plain serial host code — one loop per barcode, pair and
// read, IEEE + - * / and fma in the stated order, the log being dmx_log's host emulation (demuxlet_amd/csrc/dmx_log.hpp).  Written from
// the header's text, not from the kernels: no tiles, lanes, scans, seed tables or refined reciprocals.  Built with -ffp-contract=off it
// must give the kernels' bits (tests/test_gpu_contract_bits.py); tests/test_contract_emul_cpu.py checks it against the float64
// restatements and 50-digit arithmetic first.
//
// Three deliberately wrong variants exist so that the tests can show that their inputs tell them apart: the same source built with
// -ffp-contract=fast -DEMU_FUSE_SHARED_PRODUCTS (g++ contracts a product into a sum only when the product has no other use, and the
// three products of the genotype-likelihood recurrence are also divided on their own: alone, the flag changes nothing in the refinement
// and the cluster stage, whereas a device compiler with contraction on fuses them all the same; the macro makes that sum fused too),
// emu_set_variant(EMU_DESCENDING) (a barcode's pairs, a chunk's members, a SNP's slots, the 64 sums of the goodness of fit and of the
// share fit, and the site audit's chunk partials taken last first) and emu_set_variant(EMU_LIBM_LOG) (libm's log for dmx_log).
//
// Counters (int64[3], per call): log arguments that are zero, log arguments that are otherwise not positive normal numbers
// (subnormal, negative, inf, nan — the kernels hand both kinds to the runtime's log, the emulator to libm's), and rescales taken.
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "dmx_hyp_plan.hpp"
#include "dmx_log.hpp"

extern "C" {
typedef struct {
  int32_t n_cells, n_snps;
  const int64_t* cell_pair_off;   // [n_cells + 1]
  const int64_t* cell_read_off;   // [n_cells + 1]
  const int32_t* pair_snp;        // [n_pairs], or NULL: pair t of a barcode is SNP t
  const void* pair_nrd;           // [n_pairs] of nrd_width bytes each
  int32_t nrd_width, reserved;
  const uint8_t* reads;           // allele << 7 | base quality
} emu_pileup;
enum { EMU_DESCENDING = 1, EMU_LIBM_LOG = 2 };
}

namespace {

int g_variant = 0;
int64_t g_log_zero = 0, g_log_other = 0, g_rescales = 0;

void counters_reset() { g_log_zero = g_log_other = g_rescales = 0; }
void counters_out(int64_t* out) {
  if (out) { out[0] = g_log_zero; out[1] = g_log_other; out[2] = g_rescales; }
}

double emu_log(double x) {
  if (x == 0.0) { ++g_log_zero; return log(x); }
  if (!(x >= 0x1p-1022 && x < INFINITY)) { ++g_log_other; return log(x); }
  return (g_variant & EMU_LIBM_LOG) ? log(x) : dmx_log_host_emul(x);
}

// position i of n in the order of the contract (ascending), or of the wrong variant
int64_t at(int64_t i, int64_t n) { return (g_variant & EMU_DESCENDING) ? n - 1 - i : i; }

uint32_t nrd_of(const emu_pileup& pl, int64_t p) {
  if (pl.nrd_width == 1) return ((const uint8_t*)pl.pair_nrd)[p];
  if (pl.nrd_width == 2) return ((const uint16_t*)pl.pair_nrd)[p];
  return ((const uint32_t*)pl.pair_nrd)[p];
}

struct Pair { int32_t snp; uint32_t n; const uint8_t* rd; };

// a barcode's pairs in stored order: the reads of pair k follow those of pair k - 1
std::vector<Pair> pairs_of(const emu_pileup& pl, int32_t b) {
  std::vector<Pair> out;
  int64_t off = pl.cell_read_off[b];
  for (int64_t p = pl.cell_pair_off[b]; p < pl.cell_pair_off[b + 1]; ++p) {
    const uint32_t n = nrd_of(pl, p);
    out.push_back(Pair{pl.pair_snp ? pl.pair_snp[p] : (int32_t)(p - pl.cell_pair_off[b]), n, pl.reads + off});
    off += n;
  }
  return out;
}

// pR / pA of a stored read: the match probability for the read's own allele, a third of the error for the other
void read_factors(uint8_t byte, const double* mat, const double* err, double& pR, double& pA) {
  const int bq = byte & 127;
  const double e3 = err[bq] / 3.0;
  if (byte >> 7) { pR = e3; pA = mat[bq]; } else { pR = mat[bq]; pA = e3; }
}

bool row_nonzero(const float* r) { return r[0] != 0.f || r[1] != 0.f || r[2] != 0.f; }

double add_exponent(int32_t E, double lg) { return fma((double)E, DMX_LOG_LN2HI, fma((double)E, DMX_LOG_LN2LO, lg)); }

const double kRescaleBelow = 0x1p-300;

// ---- dmx_engine_ambient: log(gp_0 f_0 + gp_1 f_1 + gp_2 f_2) of one pair at one rho ------------------------------------------------------
double ambient_term(const Pair& pr, const float* row, double a, double rho, const double* mat, const double* err) {
  const double om = 1.0 - rho, ra = rho * a;
  const double p[3] = {ra, 0.5 * om + ra, om + ra};
  const double q[3] = {1.0 - p[0], 1.0 - p[1], 1.0 - p[2]};
  const double gp[3] = {(double)row[0], (double)row[1], (double)row[2]};
  double f[3];
  int32_t E = 0;
  for (uint32_t r = 0; r < pr.n; ++r) {
    double pR, pA;
    read_factors(pr.rd[r], mat, err, pR, pA);
    for (int g = 0; g < 3; ++g) {
      const double t = pR * q[g] + pA * p[g];
      f[g] = r == 0 ? t : f[g] * t;
    }
    if (r == 0 && pr.n >= 8)
      for (int g = 0; g < 3; ++g) if (gp[g] == 0.0) f[g] = 0.0;
    if (pr.n >= 8 && (r & 7) == 7) {
      const double mx = fmax(f[0], fmax(f[1], f[2]));
      if (mx < kRescaleBelow && mx > 0.0) {
        int e;
        (void)frexp(mx, &e);
        for (int g = 0; g < 3; ++g) f[g] = ldexp(f[g], -e);
        E += e;
        ++g_rescales;
      }
    }
  }
  const double L = gp[0] * f[0] + gp[1] * f[1] + gp[2] * f[2];
  double lg = emu_log(L);
  if (E != 0) lg = add_exponent(E, lg);
  return lg;
}

// ---- the nine read products of dmx_engine_ambient_doublet and their exponents ------------------------------------------------------------
struct Nine { double f[9]; int32_t E[9]; bool deep; };

void mix_constants(double alpha, double (&cm)[9]) {
  for (int l = 0; l < 3; ++l)
    for (int m = 0; m < 3; ++m) cm[l * 3 + m] = 0.5 * l + (m - l) * 0.5 * alpha;
}

Nine nine_products(const Pair& pr, const double (&cm)[9], double a, double rho, const double* mat, const double* err) {
  const double om = 1.0 - rho, ra = rho * a;
  double p[9], q[9];
  for (int k = 0; k < 9; ++k) { p[k] = om * cm[k] + ra; q[k] = 1.0 - p[k]; }
  Nine x;
  x.deep = pr.n >= 8;
  for (int k = 0; k < 9; ++k) { x.f[k] = 0.0; x.E[k] = 0; }
  for (uint32_t r = 0; r < pr.n; ++r) {
    double pR, pA;
    read_factors(pr.rd[r], mat, err, pR, pA);
    for (int k = 0; k < 9; ++k) {
      const double t = pR * q[k] + pA * p[k];
      x.f[k] = r == 0 ? t : x.f[k] * t;
    }
    if (x.deep && (r & 7) == 7)
      for (int k = 0; k < 9; ++k)
        if (x.f[k] < kRescaleBelow && x.f[k] > 0.0) {
          int e;
          (void)frexp(x.f[k], &e);
          x.f[k] = ldexp(x.f[k], -e);
          x.E[k] += e;
          ++g_rescales;
        }
  }
  return x;
}

// log(sum_l sum_m gp1_l gp2_m f_lm) of one candidate
double nine_fold(const Nine& x, const float* r1, const float* r2) {
  double w[9];
  for (int k = 0; k < 9; ++k) w[k] = (double)r1[k / 3] * (double)r2[k % 3];
  double L = 0.0;
  int32_t em = 0;
  if (x.deep) {
    em = INT32_MIN / 2;
    for (int k = 0; k < 9; ++k)
      if (w[k] != 0.0 && x.f[k] > 0.0 && x.E[k] > em) em = x.E[k];
    for (int k = 0; k < 9; ++k) {
      int sh = x.E[k] - em;
      if (sh < -1100) sh = -1100;
      const double t = w[k] != 0.0 ? w[k] * ldexp(x.f[k], sh) : 0.0;
      L = k == 0 ? t : L + t;
    }
  } else {
    for (int k = 0; k < 9; ++k) {
      const double t = w[k] * x.f[k];
      L = k == 0 ? t : L + t;
    }
  }
  double lg = emu_log(L);
  if (x.deep && em != 0) lg = add_exponent(em, lg);
  return lg;
}

// ---- the per-pair genotype likelihoods of the refinement and the cluster stage (the reference's recurrence) --------------------------------
void pair_gl(const Pair& pr, const double* mat, const double* err, double (&G)[3], uint32_t& alt) {
  G[0] = G[1] = G[2] = 1.0;
  alt = 0;
  for (uint32_t r = 0; r < pr.n; ++r) {
    const int bq = pr.rd[r] & 127;
    const bool a = (pr.rd[r] >> 7) != 0;
    const double m = mat[bq], e3 = err[bq] / 3.0, h = 0.5 - err[bq] / 3.0;
    alt += a;
    const double o0 = G[0], o2 = G[2], x0 = a ? e3 : m, x2 = a ? m : e3;
    G[0] *= x0;
    G[1] *= h;
    G[2] *= x2;
#ifdef EMU_FUSE_SHARED_PRODUCTS
    const double tmp = fma(o2, x2, fma(o0, x0, G[1]));   // the contraction variant only (see the head of the file)
#else
    (void)o0; (void)o2;
    const double tmp = G[0] + G[1] + G[2];
#endif
    G[0] /= tmp; G[1] /= tmp; G[2] /= tmp;
  }
  G[0] += 1e-6; G[1] += 1e-6; G[2] += 1e-6;
  const double tmp = G[0] + G[1] + G[2];
  G[0] /= tmp; G[1] /= tmp; G[2] /= tmp;
}

// ---- the per-pair terms of dmx_engine_fit, which dmx_engine_site_fit reuses operation for operation ---------------------------------------
// state 0: the pair does not count (no stored read, or an all-zero gp row of a hypothesised sample); 2: counted in n_zero; 1: it
// contributes c0, c0 + e1 and max(0, d) (the goodness of fit) and, for the site audit, k(x) - a1 and max(0, da).
struct PairFit { int state; uint32_t m, kx; double c0, e1, d, a1, da; };

PairFit fit_pair(const Pair& x, const float* g, int32_t V, int32_t v1, int32_t v2, const double (&cm)[9], double om, double rh, const double* amb,
                 int32_t M, const double* mat, const double* err) {
  PairFit out = {0, 0u, 0u, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (x.n == 0) return out;
  const bool dbl = v2 >= 0;
  const int NC = dbl ? 9 : 3;
  const float* r1 = g + ((size_t)x.snp * V + v1) * 3;
  const float* r2 = dbl ? g + ((size_t)x.snp * V + v2) * 3 : nullptr;
  if (!row_nonzero(r1) || (dbl && !row_nonzero(r2))) return out;
  double W[9], p[9], q[9];
  for (int c = 0; c < NC; ++c) W[c] = dbl ? (double)r1[c / 3] * (double)r2[c % 3] : (double)r1[c];
  const double ra = rh * (amb ? amb[x.snp] : 0.0);
  for (int c = 0; c < NC; ++c) { p[c] = om * cm[c] + ra; q[c] = 1.0 - p[c]; }
  const uint32_t m = x.n < (uint32_t)M ? x.n : (uint32_t)M;
  double t[8][9][2];
  uint32_t xobs = 0;
  for (uint32_t r = 0; r < m; ++r) {
    const int bq = x.rd[r] & 127;
    const double mt = mat[bq], e3 = err[bq] / 3.0;
    xobs |= (uint32_t)(x.rd[r] >> 7) << r;
    for (int c = 0; c < NC; ++c) {
      t[r][c][0] = mt * q[c] + e3 * p[c];
      t[r][c][1] = e3 * q[c] + mt * p[c];
    }
  }
  auto likelihood = [&](uint32_t y) {
    double L = 0.0;
    for (int c = 0; c < NC; ++c) {
      double F = t[0][c][y & 1u];
      for (uint32_t r = 1; r < m; ++r) F = F * t[r][c][(y >> r) & 1u];
      const double wf = W[c] * F;
      L = c == 0 ? wf : L + wf;
    }
    return L;
  };
  out.m = m;
  out.kx = (uint32_t)__builtin_popcount(xobs);
  const double Lx = likelihood(xobs);
  if (Lx == 0.0) { out.state = 2; return out; }
  const double c0 = emu_log(Lx);
  double S0 = 0.0, S1 = 0.0, S2 = 0.0, A1 = 0.0, A2 = 0.0;
  for (uint32_t y = 0; y < (1u << m); ++y) {
    const double L = likelihood(y);
    if (L == 0.0) continue;
    const double u = emu_log(L) - c0, ky = (double)__builtin_popcount(y);
    S0 += L; S1 += L * u; S2 += L * (u * u);
    A1 += L * ky; A2 += L * (ky * ky);
  }
  if (S0 == 0.0 || !(fabs(S0) < INFINITY)) { out.state = 2; return out; }
  out.c0 = c0;
  out.e1 = S1 / S0; out.d = S2 / S0 - out.e1 * out.e1;
  out.a1 = A1 / S0; out.da = A2 / S0 - out.a1 * out.a1;
  out.state = 1;
  return out;
}

// ---- the entries of dmx_engine_share_scan (NE = 3: l at alpha = 0) and dmx_engine_share_fit (NE = 9: k = 3 l + m) ----------------------------
// f with its exponent E and, where `diff[k]`, S1 = sum u and S2 = sum u u of u = (pA - pR) / t; rescaled after every eighth read at every depth.
const int32_t kNoExponent = INT32_MIN / 2;

struct Entries { double f[9], S1[9], S2[9]; int32_t E[9]; };

Entries share_entries(const Pair& pr, int NE, const double* c, const bool* diff, double om, double ra, const double* mat, const double* err) {
  double p[9], q[9];
  for (int k = 0; k < NE; ++k) { p[k] = om * c[k] + ra; q[k] = 1.0 - p[k]; }
  Entries x;
  for (int k = 0; k < 9; ++k) { x.f[k] = 0.0; x.S1[k] = 0.0; x.S2[k] = 0.0; x.E[k] = 0; }
  for (uint32_t r = 0; r < pr.n; ++r) {
    double pR, pA;
    read_factors(pr.rd[r], mat, err, pR, pA);
    const double dlt = pA - pR;
    for (int k = 0; k < NE; ++k) {
      const double t = pR * q[k] + pA * p[k];
      x.f[k] = r == 0 ? t : x.f[k] * t;
      if (diff[k]) {
        const double u = t != 0.0 ? dlt / t : 0.0;
        x.S1[k] += u; x.S2[k] += u * u;
      }
    }
    if ((r & 7) == 7)
      for (int k = 0; k < NE; ++k)
        if (x.f[k] < kRescaleBelow && x.f[k] > 0.0) {
          int e;
          (void)frexp(x.f[k], &e);
          x.f[k] = ldexp(x.f[k], -e);
          x.E[k] += e;
          ++g_rescales;
        }
  }
  return x;
}

// The pair's three terms from the nine scaled weighted entries T (entry order) and x, y of the six l != m entries: lg, D1, D2.
void share_pair_terms(const double (&T)[9], const double (&xs)[9], const double (&ys)[9], int32_t E, double (&term)[3]) {
  double L = 0.0, L1 = 0.0, L2 = 0.0;
  bool first = true;
  for (int k = 0; k < 9; ++k) {
    L = k == 0 ? T[k] : L + T[k];
    if (k % 4 == 0) continue;
    const double t1 = T[k] * xs[k], t2 = T[k] * ys[k];
    L1 = first ? t1 : L1 + t1;
    L2 = first ? t2 : L2 + t2;
    first = false;
  }
  double lg = emu_log(L);
  if (E != 0) lg = add_exponent(E, lg);
  const double d1 = L1 / L;
  term[0] = lg; term[1] = d1; term[2] = L2 / L - d1 * d1;
}

// One evaluation of dmx_engine_share_fit at the share alpha: (LL, LL', LL''), and the pairs / reads that contributed.
void share_evaluate(const std::vector<Pair>& pr, const float* g, int32_t V, int32_t v1, int32_t v2, double rh, const double* amb, double alpha,
                    const double* mat, const double* err, double (&res)[3], int32_t& n_snp, int32_t& n_read) {
  const double om = 1.0 - rh, s1 = om * 0.5;
  double cm[9];
  mix_constants(alpha, cm);
  bool diff[9];
  for (int k = 0; k < 9; ++k) diff[k] = k % 4 != 0;
  double sums[64][3];
  for (int l = 0; l < 64; ++l) sums[l][0] = sums[l][1] = sums[l][2] = 0.0;
  n_snp = 0; n_read = 0;
  const int64_t n = (int64_t)pr.size();
  for (int64_t i = 0; i < n; ++i) {
    const int64_t kp = at(i, n);
    const Pair& x = pr[(size_t)kp];
    if (x.n == 0) continue;
    const float* r1 = g + ((size_t)x.snp * V + v1) * 3;
    const float* r2 = g + ((size_t)x.snp * V + v2) * 3;
    if (!row_nonzero(r1) || !row_nonzero(r2)) continue;
    const double ra = rh * (amb ? amb[x.snp] : 0.0);
    const Entries e = share_entries(x, 9, cm, diff, om, ra, mat, err);
    double w[9], T[9], xs[9], ys[9];
    int32_t E = kNoExponent;
    for (int k = 0; k < 9; ++k) {
      w[k] = (double)r1[k / 3] * (double)r2[k % 3];
      if (w[k] != 0.0 && e.f[k] > 0.0 && e.E[k] > E) E = e.E[k];
    }
    for (int k = 0; k < 9; ++k) {
      int sh = e.E[k] - E;
      if (sh < -1100) sh = -1100;
      T[k] = w[k] != 0.0 ? w[k] * ldexp(e.f[k], sh) : 0.0;
      const double s = s1 * (double)(k % 3 - k / 3);
      xs[k] = s * e.S1[k];
      ys[k] = xs[k] * xs[k] - (s * s) * e.S2[k];
    }
    double term[3];
    share_pair_terms(T, xs, ys, E, term);
    const int l = (int)(kp % 64);
    for (int j = 0; j < 3; ++j) sums[l][j] += term[j];
    n_snp += 1; n_read += (int32_t)x.n;
  }
  res[0] = res[1] = res[2] = 0.0;
  for (int i = 0; i < 64; ++i) {
    const int l = (int)at(i, 64);
    for (int j = 0; j < 3; ++j) res[j] += sums[l][j];
  }
}

bool finite3(const double (&r)[3]) { return fabs(r[0]) < INFINITY && fabs(r[1]) < INFINITY && fabs(r[2]) < INFINITY; }

}  // namespace

extern "C" {

void emu_set_variant(int v) { g_variant = v; }

void emu_log_n(const double* x, double* y, int64_t n) {
  for (int64_t i = 0; i < n; ++i) y[i] = emu_log(x[i]);
}

// dmx_engine_ambient: ll[B][Q], n_snp[B], n_read[B]
void emu_ambient(const emu_pileup* pl, const float* g, int32_t V, const double* mat, const double* err, const int32_t* assign,
                 const double* amb, const double* grid, int32_t Q, double* ll, int32_t* n_snp, int32_t* n_read, int64_t* counters) {
  counters_reset();
  for (int32_t b = 0; b < pl->n_cells; ++b) {
    for (int32_t q = 0; q < Q; ++q) ll[(size_t)b * Q + q] = 0.0;
    n_snp[b] = 0; n_read[b] = 0;
    const int32_t v = assign[b];
    if (v < 0) continue;
    const std::vector<Pair> pr = pairs_of(*pl, b);
    const int64_t n = (int64_t)pr.size();
    for (int32_t q = 0; q < Q; ++q) {
      double acc = 0.0;
      int32_t ns = 0, nr = 0;
      for (int64_t i = 0; i < n; ++i) {
        const Pair& x = pr[(size_t)at(i, n)];
        const float* row = g + ((size_t)x.snp * V + v) * 3;
        if (x.n == 0 || !row_nonzero(row)) continue;
        acc += ambient_term(x, row, amb[x.snp], grid[q], mat, err);
        ns += 1; nr += (int32_t)x.n;
      }
      ll[(size_t)b * Q + q] = acc;
      n_snp[b] = ns; n_read[b] = nr;
    }
  }
  counters_out(counters);
}

// dmx_engine_ambient_doublet: ll[B][C][A][Q], n_snp[B][C], n_read[B][C]
void emu_ambient_doublet(const emu_pileup* pl, const float* g, int32_t V, const double* mat, const double* err, const int32_t* cand, int32_t C,
                         const double* alpha, int32_t A, const double* amb, const double* grid, int32_t Q, double* ll, int32_t* n_snp,
                         int32_t* n_read, int64_t* counters) {
  counters_reset();
  std::vector<double> acc((size_t)C);
  for (int32_t b = 0; b < pl->n_cells; ++b) {
    const int32_t* cd = cand + (size_t)b * C * 2;
    for (size_t i = 0; i < (size_t)C * A * Q; ++i) ll[(size_t)b * C * A * Q + i] = 0.0;
    for (int32_t c = 0; c < C; ++c) { n_snp[(size_t)b * C + c] = 0; n_read[(size_t)b * C + c] = 0; }
    const std::vector<Pair> pr = pairs_of(*pl, b);
    const int64_t n = (int64_t)pr.size();
    for (int32_t ai = 0; ai < A; ++ai) {
      double cm[9];
      mix_constants(alpha[ai], cm);
      for (int32_t q = 0; q < Q; ++q) {
        for (int32_t c = 0; c < C; ++c) acc[(size_t)c] = 0.0;
        for (int64_t i = 0; i < n; ++i) {
          const Pair& x = pr[(size_t)at(i, n)];
          if (x.n == 0) continue;
          bool any = false;
          for (int32_t c = 0; c < C && !any; ++c)
            any = cd[2 * c] >= 0 && row_nonzero(g + ((size_t)x.snp * V + cd[2 * c]) * 3) && row_nonzero(g + ((size_t)x.snp * V + cd[2 * c + 1]) * 3);
          if (!any) continue;
          const Nine f = nine_products(x, cm, amb[x.snp], grid[q], mat, err);
          for (int32_t c = 0; c < C; ++c) {
            if (cd[2 * c] < 0) continue;
            const float* r1 = g + ((size_t)x.snp * V + cd[2 * c]) * 3;
            const float* r2 = g + ((size_t)x.snp * V + cd[2 * c + 1]) * 3;
            if (!row_nonzero(r1) || !row_nonzero(r2)) continue;
            acc[(size_t)c] += nine_fold(f, r1, r2);
            if (ai == 0 && q == 0) { n_snp[(size_t)b * C + c] += 1; n_read[(size_t)b * C + c] += (int32_t)x.n; }
          }
        }
        for (int32_t c = 0; c < C; ++c)
          if (cd[2 * c] >= 0) ll[(((size_t)b * C + c) * A + ai) * Q + q] = acc[(size_t)c];
      }
    }
  }
  counters_out(counters);
}

// dmx_engine_fit: obs / mean / var [B], n_snp / n_read / n_trunc / n_zero [B]; rho / amb may be NULL (= 0)
void emu_fit(const emu_pileup* pl, const float* g, int32_t V, const double* mat, const double* err, const int32_t* hyp, const double* alpha,
             const double* rho, const double* amb, int32_t M, double* obs, double* mean, double* var, int32_t* n_snp, int32_t* n_read,
             int32_t* n_trunc, int32_t* n_zero, int64_t* counters) {
  counters_reset();
  for (int32_t b = 0; b < pl->n_cells; ++b) {
    obs[b] = mean[b] = var[b] = 0.0;
    n_snp[b] = n_read[b] = n_trunc[b] = n_zero[b] = 0;
    const int32_t v1 = hyp[2 * (size_t)b], v2 = hyp[2 * (size_t)b + 1];
    if (v1 < 0) continue;
    const bool dbl = v2 >= 0;
    const double rh = rho ? rho[b] : 0.0, om = 1.0 - rh;
    double cm[9];
    if (dbl) mix_constants(alpha[b], cm);
    else for (int c = 0; c < 3; ++c) cm[c] = 0.5 * c;
    double s_obs[64], s_mean[64], s_var[64];
    for (int l = 0; l < 64; ++l) s_obs[l] = s_mean[l] = s_var[l] = 0.0;
    const std::vector<Pair> pr = pairs_of(*pl, b);
    const int64_t n = (int64_t)pr.size();
    for (int64_t i = 0; i < n; ++i) {
      const int64_t k = at(i, n);
      const Pair& x = pr[(size_t)k];
      const PairFit f = fit_pair(x, g, V, v1, v2, cm, om, rh, amb, M, mat, err);
      if (f.state == 2) n_zero[b] += 1;
      if (f.state != 1) continue;
      const double c0 = f.c0, e1 = f.e1, d = f.d;
      const uint32_t m = f.m;
      const int l = (int)(k % 64);
      s_obs[l] += c0; s_mean[l] += c0 + e1; s_var[l] += d > 0.0 ? d : 0.0;
      n_snp[b] += 1; n_read[b] += (int32_t)m; n_trunc[b] += x.n > (uint32_t)M;
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int i = 0; i < 64; ++i) {
      const int l = (int)at(i, 64);
      a0 += s_obs[l]; a1 += s_mean[l]; a2 += s_var[l];
    }
    obs[b] = a0; mean[b] = a1; var[b] = a2;
  }
  counters_out(counters);
}

// dmx_engine_share_scan: out[B][T][V][3], n_snp_read[B][T][2]; rho / amb may be NULL (= 0)
void emu_share_scan(const emu_pileup* pl, const float* g, int32_t V, const double* mat, const double* err, const int32_t* anchors, int32_t T,
                    const double* rho, const double* amb, double* out, int32_t* n_snp_read, int64_t* counters) {
  counters_reset();
  struct ScanPair { bool used; int32_t snp, E; double g1[3], F[3], xs[9], ys[9]; };
  const double c[3] = {0.0, 0.5, 1.0};               // c_l = 0.5 l
  const bool diff[3] = {true, true, true};
  for (int32_t b = 0; b < pl->n_cells; ++b) {
    const std::vector<Pair> pr = pairs_of(*pl, b);
    const int64_t n = (int64_t)pr.size();
    const double rh = rho ? rho[b] : 0.0, om = 1.0 - rh, s1 = om * 0.5;
    for (int32_t t = 0; t < T; ++t) {
      const size_t slot = (size_t)b * T + t;
      for (size_t i = 0; i < (size_t)V * 3; ++i) out[slot * V * 3 + i] = 0.0;
      n_snp_read[2 * slot] = n_snp_read[2 * slot + 1] = 0;
      const int32_t a = anchors[slot];
      if (a < 0) continue;
      std::vector<ScanPair> sp((size_t)n);
      for (int64_t i = 0; i < n; ++i) {              // the read loop: once per pair for all partners
        const Pair& x = pr[(size_t)i];
        ScanPair& h = sp[(size_t)i];
        h.used = false;
        const float* r1 = g + ((size_t)x.snp * V + a) * 3;
        if (x.n == 0 || !row_nonzero(r1)) continue;
        h.used = true; h.snp = x.snp;
        n_snp_read[2 * slot] += 1; n_snp_read[2 * slot + 1] += (int32_t)x.n;
        const double ra = rh * (amb ? amb[x.snp] : 0.0);
        const Entries e = share_entries(x, 3, c, diff, om, ra, mat, err);
        h.E = kNoExponent;
        for (int l = 0; l < 3; ++l) {
          h.g1[l] = (double)r1[l];
          if (h.g1[l] != 0.0 && e.f[l] > 0.0 && e.E[l] > h.E) h.E = e.E[l];
        }
        for (int l = 0; l < 3; ++l) {
          int sh = e.E[l] - h.E;
          if (sh < -1100) sh = -1100;
          h.F[l] = (h.g1[l] != 0.0 && e.f[l] > 0.0) ? ldexp(e.f[l], sh) : 0.0;
        }
        for (int k = 0; k < 9; ++k) {
          const int l = k / 3, m = k % 3;
          const double s = s1 * (double)(m - l);
          h.xs[k] = s * e.S1[l];
          h.ys[k] = h.xs[k] * h.xs[k] - (s * s) * e.S2[l];
        }
      }
      for (int32_t v = 0; v < V; ++v) {
        if (v == a) continue;
        double acc[3] = {0.0, 0.0, 0.0};
        for (int64_t i = 0; i < n; ++i) {
          const ScanPair& h = sp[(size_t)at(i, n)];
          if (!h.used) continue;
          const float* r2 = g + ((size_t)h.snp * V + v) * 3;
          if (!row_nonzero(r2)) continue;
          double T9[9];
          for (int k = 0; k < 9; ++k) {
            const double w = h.g1[k / 3] * (double)r2[k % 3];
            T9[k] = w != 0.0 ? w * h.F[k / 3] : 0.0;
          }
          double term[3];
          share_pair_terms(T9, h.xs, h.ys, h.E, term);
          for (int j = 0; j < 3; ++j) acc[j] += term[j];
        }
        for (int j = 0; j < 3; ++j) out[(slot * V + v) * 3 + j] = acc[j];
      }
    }
  }
  counters_out(counters);
}

// dmx_engine_share_fit: values[B][C][13], counts[B][C][4]; rho / amb may be NULL (= 0).  trace[B][C][3] (may be NULL; the tests' conditions
// on their inputs, not an output of the pass): how the driver left (1 = the non-finite exit, 2 / 3 / 4 = that step, 10 = iterated), the
// bisection steps it took, and those of them where a Newton step had been formed (LL'' < 0) and was refused.
void emu_share_fit(const emu_pileup* pl, const float* g, int32_t V, const double* mat, const double* err, const int32_t* cand, int32_t C,
                   const double* rho, const double* amb, double start, double tol, int32_t max_iter, double probe, double* values,
                   int32_t* counts, int32_t* trace, int64_t* counters) {
  counters_reset();
  enum { INTERIOR = 1, AT_0 = 2, AT_1 = 4, NOT_CONVERGED = 8, FLAT = 16, NONFINITE = 32 };
  for (int32_t b = 0; b < pl->n_cells; ++b) {
    const std::vector<Pair> pr = pairs_of(*pl, b);
    const double rh = rho ? rho[b] : 0.0;
    for (int32_t c = 0; c < C; ++c) {
      const size_t slot = (size_t)b * C + c;
      double* val = values + slot * 13;
      int32_t* cnt = counts + slot * 4;
      for (int i = 0; i < 13; ++i) val[i] = 0.0;
      cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
      if (trace) trace[3 * slot] = trace[3 * slot + 1] = trace[3 * slot + 2] = 0;
      const int32_t v1 = cand[2 * slot], v2 = cand[2 * slot + 1];
      if (v1 < 0) continue;
      auto evaluate = [&](double al, double (&res)[3], int32_t& ns, int32_t& nr) {
        share_evaluate(pr, g, V, v1, v2, rh, amb, al, mat, err, res, ns, nr);
      };
      double r0[3], r1[3], rx[3], rp[3] = {0.0, 0.0, 0.0};
      int32_t n_snp, n_read, ns, nr, n_eval = 0, status = 0, how = 10, n_bisect = 0, n_refused = 0;
      double ahat;
      evaluate(0.0, r0, n_snp, n_read); ++n_eval;                               // step 1
      evaluate(1.0, r1, ns, nr); ++n_eval;
      const bool dn0 = r0[1] <= 0.0, up1 = r1[1] >= 0.0;
      int end = -1;
      if (!finite3(r0) || !finite3(r1)) { end = 0; how = 1; }                   // nothing is iterated
      else if (dn0 && up1) { end = r1[0] > r0[0] ? 1 : 0; how = 2; }            // step 2
      else if (dn0) { end = 0; how = 3; }                                       // step 3
      else if (up1) { end = 1; how = 4; }                                       // step 4
      if (end == 0) { ahat = 0.0; status = AT_0; for (int j = 0; j < 3; ++j) rx[j] = r0[j]; }
      else if (end == 1) { ahat = 1.0; status = AT_1; for (int j = 0; j < 3; ++j) rx[j] = r1[j]; }
      else {
        double lo = 0.0, hi = 1.0, a = start;                                   // step 5
        for (int32_t it = 1;; ++it) {
          double r[3];
          evaluate(a, r, ns, nr); ++n_eval;                                     // step 6
          if (r[1] > 0.0) lo = a; else hi = a;                                  // step 7
          double an = a - r[1] / r[2];                                          // step 8
          if (!(r[2] < 0.0 && lo < an && an < hi)) { an = (lo + hi) / 2.0; ++n_bisect; n_refused += r[2] < 0.0; }
          const bool conv = fabs(an - a) <= tol;                                // step 9
          a = an;
          if (conv) break;
          if (it >= max_iter) { status |= NOT_CONVERGED; break; }
        }
        evaluate(a, rx, ns, nr); ++n_eval;                                      // step 10
        ahat = a; status |= INTERIOR;
      }
      if (probe >= 0.0) evaluate(probe, rp, ns, nr);                            // not counted in n_eval
      if (rx[2] >= 0.0) status |= FLAT;
      if (!finite3(r0) || !finite3(r1) || !finite3(rx)) status |= NONFINITE;
      val[0] = ahat;
      for (int j = 0; j < 3; ++j) { val[1 + j] = rx[j]; val[4 + j] = r0[j]; val[7 + j] = r1[j]; val[10 + j] = rp[j]; }
      cnt[0] = n_eval; cnt[1] = status; cnt[2] = n_snp; cnt[3] = n_read;
      if (trace) { trace[3 * slot] = how; trace[3 * slot + 1] = n_bisect; trace[3 * slot + 2] = n_refused; }
    }
  }
  counters_out(counters);
}

// dmx_engine_site_fit: obs / mean / var / exc / vexc [S], n_cell / n_read / n_alt / n_trunc / n_zero [S]  (S = the genotype matrix's SNPs)
void emu_site_fit(const emu_pileup* pl, const float* g, int32_t S, int32_t V, const double* mat, const double* err, const int32_t* hyp,
                  const double* alpha, const double* rho, const double* amb, int32_t M, double* obs, double* mean, double* var, double* exc,
                  double* vexc, int32_t* n_cell, int32_t* n_read, int32_t* n_alt, int32_t* n_trunc, int32_t* n_zero, int64_t* counters) {
  counters_reset();
  double* val[5] = {obs, mean, var, exc, vexc};
  int32_t* cnt[5] = {n_cell, n_read, n_alt, n_trunc, n_zero};
  for (int32_t i = 0; i < S; ++i)
    for (int j = 0; j < 5; ++j) { val[j][i] = 0.0; cnt[j][i] = 0; }
  std::vector<std::vector<int32_t>> chunks;         // the engine's own list (singlets, then doublets); no chunk straddles the two kinds
  std::vector<int32_t> used;
  int32_t n_sng = 0;
  if (dmx::hyp_list_used(hyp, pl->n_cells, V, used, &n_sng) >= 0) { counters_out(counters); return; }   // (a table that the engine refuses)
  for (int kind = 0; kind < 2; ++kind) {
    const std::vector<int32_t> list(kind == 0 ? used.begin() : used.begin() + n_sng, kind == 0 ? used.begin() + n_sng : used.end());
    for (size_t c0 = 0; c0 < list.size(); c0 += 64)
      chunks.emplace_back(list.begin() + (int64_t)c0, list.begin() + (int64_t)(c0 + 64 < list.size() ? c0 + 64 : list.size()));
  }
  const int64_t nch = (int64_t)chunks.size();
  std::vector<double> part((size_t)nch * S * 5, 0.0);
  for (int64_t ch = 0; ch < nch; ++ch) {
    const std::vector<int32_t>& mem = chunks[(size_t)ch];
    const int64_t nm = (int64_t)mem.size();
    double* pv = part.data() + (size_t)ch * S * 5;
    for (int64_t i = 0; i < nm; ++i) {
      const int32_t b = mem[(size_t)at(i, nm)];
      const int32_t v1 = hyp[2 * (size_t)b], v2 = hyp[2 * (size_t)b + 1];
      const double rh = rho ? rho[b] : 0.0, om = 1.0 - rh;
      double cm[9];
      if (v2 >= 0) mix_constants(alpha[b], cm);
      else for (int c = 0; c < 3; ++c) cm[c] = 0.5 * c;
      for (const Pair& x : pairs_of(*pl, b)) {
        if (x.snp < 0 || x.snp >= S) continue;
        const PairFit f = fit_pair(x, g, V, v1, v2, cm, om, rh, amb, M, mat, err);
        if (f.state == 2) n_zero[x.snp] += 1;
        if (f.state != 1) continue;
        double* o = pv + (size_t)x.snp * 5;
        o[0] += f.c0; o[1] += f.c0 + f.e1; o[2] += f.d > 0.0 ? f.d : 0.0;
        o[3] += (double)f.kx - f.a1; o[4] += f.da > 0.0 ? f.da : 0.0;
        n_cell[x.snp] += 1; n_read[x.snp] += (int32_t)f.m; n_alt[x.snp] += (int32_t)f.kx; n_trunc[x.snp] += x.n > (uint32_t)M;
      }
    }
  }
  for (int64_t i = 0; i < nch; ++i) {
    const double* pv = part.data() + (size_t)at(i, nch) * S * 5;
    for (int32_t s = 0; s < S; ++s)
      for (int j = 0; j < 5; ++j) val[j][s] += pv[(size_t)s * 5 + j];
  }
  counters_out(counters);
}

// dmx_engine_refine_genotypes: ll[S][V][3], n_cell / n_ref / n_alt [S][V]  (S = the genotype matrix's SNPs)
void emu_refine(const emu_pileup* pl, int32_t S, int32_t V, const double* mat, const double* err, const int32_t* assign, double* ll,
                int32_t* n_cell, int32_t* n_ref, int32_t* n_alt, int64_t* counters) {
  counters_reset();
  const size_t rows = (size_t)S * V;
  for (size_t o = 0; o < rows; ++o) { ll[3 * o] = ll[3 * o + 1] = ll[3 * o + 2] = 0.0; n_cell[o] = n_ref[o] = n_alt[o] = 0; }
  std::vector<double> part((size_t)S * 3);
  for (int32_t v = 0; v < V; ++v) {
    std::vector<int32_t> mem;
    for (int32_t b = 0; b < pl->n_cells; ++b) if (assign[b] == v) mem.push_back(b);
    for (size_t c0 = 0; c0 < mem.size(); c0 += 64) {
      const int64_t nm = (int64_t)(mem.size() - c0 < 64 ? mem.size() - c0 : 64);
      for (double& x : part) x = 0.0;
      for (int64_t i = 0; i < nm; ++i) {
        const int32_t b = mem[c0 + (size_t)at(i, nm)];
        for (const Pair& x : pairs_of(*pl, b)) {
          if (x.snp < 0 || x.snp >= S) continue;
          double G[3];
          uint32_t alt;
          pair_gl(x, mat, err, G, alt);
          const size_t o = (size_t)x.snp * V + v;
          for (int gg = 0; gg < 3; ++gg) part[(size_t)x.snp * 3 + gg] += emu_log(G[gg]);
          n_cell[o] += 1; n_ref[o] += (int32_t)(x.n - alt); n_alt[o] += (int32_t)alt;
        }
      }
      for (int32_t i = 0; i < S; ++i)
        for (int gg = 0; gg < 3; ++gg) ll[((size_t)i * V + v) * 3 + gg] += part[(size_t)i * 3 + gg];
    }
  }
  counters_out(counters);
}

// dmx_engine_cluster_stage: snp_off[S + 1], cell[P], lgl[P][3], ref_alt[P]  (S = the pileup's SNPs)
void emu_cluster_stage(const emu_pileup* pl, const double* mat, const double* err, int64_t* snp_off, int32_t* cell, double* lgl,
                       uint32_t* ref_alt, int64_t* counters) {
  counters_reset();
  const int32_t S = pl->n_snps;
  for (int32_t i = 0; i <= S; ++i) snp_off[i] = 0;
  for (int32_t b = 0; b < pl->n_cells; ++b)
    for (const Pair& x : pairs_of(*pl, b)) snp_off[x.snp + 1] += 1;
  for (int32_t i = 0; i < S; ++i) snp_off[i + 1] += snp_off[i];
  std::vector<int64_t> next(snp_off, snp_off + S);
  for (int32_t b = 0; b < pl->n_cells; ++b)            // ascending cell id: a SNP's slots come out in that order
    for (const Pair& x : pairs_of(*pl, b)) {
      const int64_t j = next[(size_t)x.snp]++;
      double G[3];
      uint32_t alt;
      pair_gl(x, mat, err, G, alt);
      for (int gg = 0; gg < 3; ++gg) lgl[3 * j + gg] = emu_log(G[gg]);
      ref_alt[j] = (x.n - alt) | (alt << 16);
      cell[j] = b;
    }
  counters_out(counters);
}

// dmx_engine_cluster_mstep: LL[S][C][3], W[S][C] from the stage cache and w[B][C]
void emu_cluster_mstep(int32_t S, int32_t C, const int64_t* snp_off, const int32_t* cell, const double* lgl, const double* w, double* LL,
                       double* W) {
  for (int32_t i = 0; i < S; ++i)
    for (int32_t c = 0; c < C; ++c) {
      double a[3] = {0.0, 0.0, 0.0}, ws = 0.0;
      const int64_t n = snp_off[i + 1] - snp_off[i];
      for (int64_t t = 0; t < n; ++t) {
        const int64_t j = snp_off[i] + at(t, n);
        const double x = w[(size_t)cell[j] * C + c];
        for (int gg = 0; gg < 3; ++gg) a[gg] = fma(x, lgl[3 * j + gg], a[gg]);
        ws += x;
      }
      const size_t o = (size_t)i * C + c;
      LL[3 * o] = a[0]; LL[3 * o + 1] = a[1]; LL[3 * o + 2] = a[2]; W[o] = ws;
    }
}

}  // extern "C"
