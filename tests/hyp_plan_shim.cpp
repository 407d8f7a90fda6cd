// Test helper (CPU): a C entry to demuxlet_amd/csrc/dmx_hyp_plan.hpp for tests/test_hyp_plan_cpu.py.  No HIP.
#include "dmx_hyp_plan.hpp"

// idx[B] receives the list; returns the first bad barcode or -1, *n_used and *n_sng as the function left them (0 where it refused).
extern "C" int32_t hyp_plan_list(const int32_t* hyp, int32_t B, int32_t V, int32_t* idx, int32_t* n_used, int32_t* n_sng) {
  std::vector<int32_t> v;
  *n_used = 0; *n_sng = 0;
  const int32_t bad = dmx::hyp_list_used(hyp, B, V, v, n_sng);
  if (bad >= 0) { *n_sng = 0; return bad; }
  *n_used = (int32_t)v.size();
  for (std::size_t k = 0; k < v.size(); ++k) idx[k] = v[k];
  return -1;
}
