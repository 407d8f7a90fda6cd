// The list of used barcodes of a hypothesis table (host only, plain C++: the engine and the tests' host emulator share it).
// hyp[B][2] holds per barcode (-1, .) = unused, (v, -1) = the singlet of sample v, (v1, v2) = the doublet of two different samples.
// The order is contract (include/dmx.h: the site audit sums "the used barcodes as dmx_engine_fit lists them"): the singlets in
// ascending cell id, then the doublets in ascending cell id.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace dmx {

// Fills idx with the used barcodes and *n_sng with the number of singlets among them; returns -1.  Where a hypothesis is not -1, a
// sample in [0, V) or two different samples, returns the first such barcode instead (idx and *n_sng are then unspecified).
inline int32_t hyp_list_used(const int32_t* hyp, int32_t B, int32_t V, std::vector<int32_t>& idx, int32_t* n_sng) {
  idx.clear();
  idx.reserve((std::size_t)B);
  for (int32_t b = 0; b < B; ++b) {
    const int32_t v1 = hyp[2 * (std::size_t)b], v2 = hyp[2 * (std::size_t)b + 1];
    const bool ok = v1 == -1 || (v1 >= 0 && v1 < V && (v2 == -1 || (v2 >= 0 && v2 < V && v2 != v1)));
    if (!ok) return b;
    if (v1 >= 0 && v2 < 0) idx.push_back(b);
  }
  *n_sng = (int32_t)idx.size();
  for (int32_t b = 0; b < B; ++b)
    if (hyp[2 * (std::size_t)b] >= 0 && hyp[2 * (std::size_t)b + 1] >= 0) idx.push_back(b);
  return -1;
}

}  // namespace dmx
