// Test helper (CPU): dmx_log2 as one function (dmx_log2_core) and in its two parts (dmx_log2_request, then dmx_log2_finish), on the host
// (demuxlet_amd/csrc/dmx_log.hpp; fma via libm's correctly-rounded fma()).
#include "dmx_log.hpp"
extern "C" void dmx_log2_whole_n(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = dmx_log2_host_emul(x[i]); }
extern "C" void dmx_log2_split_n(const double* x, double* y, long n) { for (long i = 0; i < n; ++i) y[i] = dmx_log2_split_host_emul(x[i]); }
