// Test helper (CPU): dmx_log2 of a mirrored pair (dmx_log2_request_mirror, dmx_log2_finish_mirror and the whole evaluation behind a failed guard, as the
// device callers combine them) and dmx_log2_core on one argument, on the host (demuxlet_amd/csrc/dmx_log.hpp; fma via libm's correctly-rounded fma()).
#include "dmx_log.hpp"
extern "C" void dmx_log2_whole_n(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = dmx_log2_host_emul(x[i]); }
extern "C" void dmx_log2_mirror_n(const double* x, const double* xm, double* y, double* ym, int* fell_back, long n) {
  for (long i = 0; i < n; ++i) fell_back[i] = dmx_log2_mirror_host_emul(x[i], xm[i], &y[i], &ym[i]);
}
