// The joint-genotype-table contract of include/dmx.h ("Joint genotype tables") as serial host code: the row transform, the weight on the
// A side, and one ascending std::fma chain per entry.  Built with -ffp-contract=off by tests/kin_ref.py.
// kin_set_variant: 0 = the contract; 1 = the SNPs in descending order; 2 = a separate multiply and add.  Both are wrong on purpose.
#include <cmath>
#include <cstdint>

namespace {
int g_variant = 0;
}

extern "C" {

void kin_set_variant(int v) { g_variant = v; }

// img[n][4] = c_i * (p0, p1, p2, m) of g[n][3], n = S * V rows, row t at SNP t / V; c may be null (no multiplication at all);
// valid[n] = 1 for a valid row
void kin_rows(const float* g, int64_t n, int32_t V, const double* c, double* img, uint8_t* valid) {
  for (int64_t t = 0; t < n; ++t) {
    const float f0 = g[3 * t], f1 = g[3 * t + 1], f2 = g[3 * t + 2];
    const double g0 = (double)f0, g1 = (double)f1, g2 = (double)f2;
    const double s = (g0 + g1) + g2;
    const bool ok = std::isfinite(s) && s > 0.0 && f0 >= 0.f && f1 >= 0.f && f2 >= 0.f;
    double r[4] = {0.0, 0.0, 0.0, 0.0};
    if (ok) { r[0] = g0 / s; r[1] = g1 / s; r[2] = g2 / s; r[3] = 1.0; }
    if (c) for (int x = 0; x < 4; ++x) r[x] = c[t / V] * r[x];
    for (int x = 0; x < 4; ++x) img[4 * t + x] = r[x];
    if (valid) valid[t] = ok ? 1 : 0;
  }
}

// T[VA][VB][4][4] from the images wa[S][VA][4] and rb[S][VB][4]
void kin_table(const double* wa, const double* rb, int32_t S, int32_t VA, int32_t VB, double* T) {
  for (int32_t a = 0; a < VA; ++a)
    for (int32_t b = 0; b < VB; ++b)
      for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 4; ++y) {
          double acc = 0.0;
          for (int32_t k = 0; k < S; ++k) {
            const int32_t i = g_variant == 1 ? S - 1 - k : k;
            const double u = wa[((int64_t)i * VA + a) * 4 + x], v = rb[((int64_t)i * VB + b) * 4 + y];
            if (g_variant == 2) {
              const double prod = u * v;
              acc = acc + prod;
            } else {
              acc = std::fma(u, v, acc);
            }
          }
          T[(((int64_t)a * VB + b) * 4 + x) * 4 + y] = acc;
        }
}

}  // extern "C"
