// BGZF members inflated on the device (dmx_inflater_*).  Included into dmx_engine.hip after the other feature
// headers; it shares nothing with the engine but set_error and HIP_TRY.
//
// k_bgzf_inflate: ONE WAVEFRONT PER MEMBER (a workgroup is one wavefront, so nothing here needs a workgroup barrier).  The decoder
// is dmx_inflate_core.hpp's, instantiated with a policy whose tables and code-length arrays are LDS (14 408 bytes per wavefront at
// the host's roots of 10 and 8) and whose output is the member's own range of the batch's device buffer.  The decoder's state — bit
// buffer, positions, the symbol in hand — is wave-uniform: every lane computes it from the same loads (a load of one address by
// 64 lanes is one broadcast), so every branch is taken by all lanes or by none and no lane ever waits for another.  The bulk
// operations spread over the lanes:
//   table fill      entry i of a strided run goes to lane (i - first) / step mod 64;
//   literal         lane 0 stores the byte;
//   match copy      lane i writes out[pos + i] from out[pos - dist + (dist < len ? i mod dist : i)], i += 64: every source byte lies
//                   before pos, that is, it was written by an EARLIER instruction of this same wavefront;
//   stored block    lane i copies byte i, i += 64.
// A wavefront's vector memory instructions reach its CU's vector cache in program order and LDS instructions execute in order, so a
// byte (or table entry) stored by one lane is what a later load of any lane of the same wavefront returns; wavefront-scope fences
// and wave barriers after the stores and before the loads pin the same order for the compiler (they emit no instruction).  No other
// wavefront ever reads or writes a member's output range, tables or status.
// Bounds: the core checks every output range against [0, out_len) and every input word against the member's padded slot before the
// policy is called; the kernel checks the member's slot and range against the batch buffers' sizes before it starts (the host has
// checked the same, so that is a second fence, not a code path).  Results are written with ordinary vector stores.
#pragma once
#include <atomic>
#include "dmx_inflate_core.hpp"

namespace dmx_gz {

struct WaveLds {
  uint32_t lit[dmxzc::kLitCap];
  uint32_t dist[dmxzc::kDistCap];
  uint32_t ct[dmxzc::kClCap];
  uint8_t submax[dmxzc::kSubmaxCap];
  uint8_t lens[(dmxzc::kLensCap + 7) & ~7u];
  uint8_t cl[32];
  uint16_t count[dmxzc::kCountCap];
};

struct WavePolicy {
  uint32_t *lit, *dist, *ct;
  uint8_t *lens, *submax, *cl;
  uint16_t* count;
  uint8_t* out;
  uint32_t lane;
  __device__ void sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
  __device__ void fill32(uint32_t* t, uint32_t first, uint32_t step, uint32_t limit, uint32_t v) { for (uint32_t i = first + lane * step; i < limit; i += 64u * step) t[i] = v; }
  __device__ void fill16(uint16_t* t, uint32_t n, uint16_t v) { for (uint32_t i = lane; i < n; i += 64u) t[i] = v; }
  __device__ void fill8(uint8_t* t, uint32_t n, uint8_t v) { for (uint32_t i = lane; i < n; i += 64u) t[i] = v; }
  // Output bytes cross lanes (a byte stored by one lane is a later match's source on another): every store is followed by a
  // wavefront-scope release and a match's loads are preceded by an acquire, with a wave barrier, so the order the hardware keeps is
  // also the order the compiler must keep.  Both fences cost no instruction at this scope.
  __device__ void published() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); }
  __device__ void put(uint32_t pos, uint8_t v) { if (lane == 0) out[pos] = v; published(); }
  __device__ void copy_in(uint32_t pos, const uint8_t* src, uint32_t n) { for (uint32_t i = lane; i < n; i += 64u) out[pos + i] = src[i]; published(); }
  __device__ void copy_match(uint32_t pos, uint32_t d, uint32_t len) {
    __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint8_t* src = out + (pos - d);
    if (d >= len) { for (uint32_t i = lane; i < len; i += 64u) out[pos + i] = src[i]; }
    else { for (uint32_t i = lane; i < len; i += 64u) out[pos + i] = src[i % d]; }
    published();
  }
};

// desc[m] = (in_off, in_len, out_off, out_len): offsets into d_in / d_out.  in_len = 0xffffffff marks a member the host refused by size.
__global__ __launch_bounds__(64) void k_bgzf_inflate(const uint8_t* __restrict__ d_in, uint32_t in_cap, uint8_t* d_out, uint32_t out_cap,
                                                     const uint4* __restrict__ desc, int32_t* __restrict__ status, int32_t n) {
  __shared__ WaveLds s;
  const int32_t m = (int32_t)blockIdx.x;
  if (m >= n) return;
  const uint4 q = desc[m];
  const uint32_t lane = threadIdx.x & 63u;
  int32_t st = dmxzc::ST_LIMIT;
  const bool fits = q.y <= dmxzc::kMaxIn && q.w <= dmxzc::kMaxOut && (q.x & 3u) == 0 && q.x <= in_cap && ((q.y + 11u) & ~3u) <= in_cap - q.x &&
                    q.z <= out_cap && q.w <= out_cap - q.z;
  if (fits) {
    WavePolicy p;
    p.lit = s.lit; p.dist = s.dist; p.ct = s.ct; p.lens = s.lens; p.submax = s.submax; p.cl = s.cl; p.count = s.count;
    p.out = d_out + q.z; p.lane = lane;
    st = dmxzc::inflate_member(p, reinterpret_cast<const uint32_t*>(d_in + q.x), q.y, q.w);
  }
  if (lane == 0) status[m] = st;
}

}  // namespace dmx_gz

// ---- the C-ABI ------------------------------------------------------------------------------------------------------
struct dmx_inflater {
  int device = 0;
  int32_t max_members = 0;
  int64_t max_in = 0, max_out = 0;
  struct Slot {
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // before H2D, after H2D, after the kernel, after D2H
    uint8_t *d_in = nullptr, *d_out = nullptr;
    uint4 *d_desc = nullptr, *h_desc = nullptr;
    int32_t *d_status = nullptr, *h_status = nullptr;
    int32_t n = 0;
    bool busy = false;
    int64_t h2d_bytes = 0, d2h_bytes = 0;
  } slot[2];
};

static std::atomic<int> g_inflater_device{-1};     // the device of the inflater created last: where a calling thread's page-locking goes

extern "C" int dmx_inflater_free(dmx_inflater* h) {
  if (!h) return DMX_OK;
  (void)hipSetDevice(h->device);
  for (dmx_inflater::Slot& s : h->slot) {
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    for (hipEvent_t& e : s.ev) if (e) (void)hipEventDestroy(e);
    if (s.d_in) (void)hipFree(s.d_in);
    if (s.d_out) (void)hipFree(s.d_out);
    if (s.d_desc) (void)hipFree(s.d_desc);
    if (s.d_status) (void)hipFree(s.d_status);
    if (s.h_desc) (void)hipHostFree(s.h_desc);
    if (s.h_status) (void)hipHostFree(s.h_status);
    if (s.stream) (void)hipStreamDestroy(s.stream);
  }
  delete h;
  return DMX_OK;
}

extern "C" int dmx_inflater_create(int32_t device, int32_t max_members, int64_t max_in_bytes, int64_t max_out_bytes, dmx_inflater** out) {
  const char* fn = "dmx_inflater_create";
  if (!out) return set_error(DMX_ERR_ARG, "%s: null argument", fn);
  *out = nullptr;
  if (max_members < 1 || max_members > (1 << 20)) return set_error(DMX_ERR_ARG, "%s: max_members %d not in [1, 2^20]", fn, max_members);
  if (max_in_bytes < 16 || max_in_bytes > ((int64_t)1 << 31) || max_out_bytes < 1 || max_out_bytes > ((int64_t)1 << 31))
    return set_error(DMX_ERR_ARG, "%s: max_in_bytes %lld / max_out_bytes %lld not in [16, 2^31] / [1, 2^31]", fn, (long long)max_in_bytes, (long long)max_out_bytes);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_error(DMX_ERR_NOGPU, "%s: no HIP device is visible (this library has no CPU fallback)", fn);
  if (device < 0 || device >= ndev) return set_error(DMX_ERR_ARG, "%s: device %d of %d", fn, device, ndev);
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_error(DMX_ERR_NOGPU, "%s: device %d is %s; this library is built for gfx950 (MI355X) only", fn, device, prop.gcnArchName);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const int64_t want = 2 * (max_in_bytes + max_out_bytes + (int64_t)max_members * 20);
  if ((int64_t)free_b < want + ((int64_t)64 << 20)) return set_error(DMX_ERR_NOMEM, "%s: %lld bytes of batch buffers do not fit the free device memory (%lld)", fn, (long long)want, (long long)free_b);
  dmx_inflater* h = new (std::nothrow) dmx_inflater;
  if (!h) return set_error(DMX_ERR_NOMEM, "%s: out of memory", fn);
  h->device = device; h->max_members = max_members; h->max_in = max_in_bytes; h->max_out = max_out_bytes;
  auto fail = [&](hipError_t e, const char* what) {
    const int code = e == hipErrorOutOfMemory ? DMX_ERR_NOMEM : DMX_ERR_HIP;
    (void)hipGetLastError();
    dmx_inflater_free(h);
    return set_error(code, "%s: %s failed: %s", fn, what, hipGetErrorString(e));
  };
  for (dmx_inflater::Slot& s : h->slot) {
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreateWithFlags");
    for (hipEvent_t& ev : s.ev) if ((e = hipEventCreate(&ev)) != hipSuccess) return fail(e, "hipEventCreate");
    if ((e = hipMalloc((void**)&s.d_in, (size_t)max_in_bytes)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipMalloc((void**)&s.d_out, (size_t)max_out_bytes)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipMalloc((void**)&s.d_desc, sizeof(uint4) * (size_t)max_members)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipMalloc((void**)&s.d_status, sizeof(int32_t) * (size_t)max_members)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipHostMalloc((void**)&s.h_desc, sizeof(uint4) * (size_t)max_members, hipHostMallocDefault)) != hipSuccess) return fail(e, "hipHostMalloc");
    if ((e = hipHostMalloc((void**)&s.h_status, sizeof(int32_t) * (size_t)max_members, hipHostMallocDefault)) != hipSuccess) return fail(e, "hipHostMalloc");
  }
  g_inflater_device = device;
  *out = h;
  return DMX_OK;
}

extern "C" int dmx_inflater_pin(void* ptr, int64_t bytes) {
  if (!ptr || bytes < 1) return set_error(DMX_ERR_ARG, "dmx_inflater_pin: null pointer or no bytes");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return set_error(DMX_ERR_NOGPU, "dmx_inflater_pin: no HIP device is visible");
  if (const int d = g_inflater_device.load(); d >= 0 && d < ndev) HIP_TRY(hipSetDevice(d));      // (not the calling thread's default device)
  const hipError_t e = hipHostRegister(ptr, (size_t)bytes, hipHostRegisterPortable);
  if (e != hipSuccess) { (void)hipGetLastError(); return set_error(e == hipErrorOutOfMemory ? DMX_ERR_NOMEM : DMX_ERR_HIP, "dmx_inflater_pin: hipHostRegister failed: %s", hipGetErrorString(e)); }
  return DMX_OK;
}

extern "C" int dmx_inflater_unpin(void* ptr) {
  if (!ptr) return DMX_OK;
  const hipError_t e = hipHostUnregister(ptr);
  if (e != hipSuccess) { (void)hipGetLastError(); return set_error(DMX_ERR_HIP, "dmx_inflater_unpin: hipHostUnregister failed: %s", hipGetErrorString(e)); }
  return DMX_OK;
}

static int submit_enqueue(dmx_inflater* h, dmx_inflater::Slot& s, int32_t n, const uint8_t* in, const int64_t* in_off, uint8_t* out, const int64_t* out_off,
                          const int32_t* out_len, bool any, int64_t ilo, int64_t ihi, int64_t olo, int64_t ohi);

extern "C" int dmx_inflater_submit(dmx_inflater* h, int32_t slot, int32_t n, const uint8_t* in, const int64_t* in_off, const int32_t* in_len,
                                   uint8_t* out, const int64_t* out_off, const int32_t* out_len) {
  const char* fn = "dmx_inflater_submit";
  if (!h) return set_error(DMX_ERR_ARG, "%s: null inflater", fn);
  if (slot < 0 || slot > 1) return set_error(DMX_ERR_ARG, "%s: slot %d is not 0 or 1", fn, slot);
  dmx_inflater::Slot& s = h->slot[slot];
  if (s.busy) return set_error(DMX_ERR_STATE, "%s: slot %d has a batch in flight (dmx_inflater_wait first)", fn, slot);
  if (n < 0 || n > h->max_members) return set_error(DMX_ERR_ARG, "%s: n %d not in [0, max_members %d]", fn, n, h->max_members);
  if (n > 0 && (!in || !in_off || !in_len || !out || !out_off || !out_len)) return set_error(DMX_ERR_ARG, "%s: null argument", fn);
  int64_t ilo = INT64_MAX, ihi = 0, olo = INT64_MAX, ohi = 0;
  for (int32_t i = 0; i < n; ++i) {
    if (in_len[i] < 0 || out_len[i] < 0 || in_off[i] < 0 || out_off[i] < 0) return set_error(DMX_ERR_ARG, "%s: member %d has a negative offset or length", fn, i);
    if ((in_off[i] & 3) != 0) return set_error(DMX_ERR_ARG, "%s: member %d: in_off %lld is not a multiple of 4", fn, i, (long long)in_off[i]);
    if ((uint32_t)in_len[i] > dmxzc::kMaxIn || (uint32_t)out_len[i] > dmxzc::kMaxOut) continue;     // refused, not an error
    ilo = std::min(ilo, in_off[i]); ihi = std::max(ihi, in_off[i] + (((int64_t)in_len[i] + 11) & ~(int64_t)3));
    olo = std::min(olo, out_off[i]); ohi = std::max(ohi, out_off[i] + out_len[i]);
  }
  const bool any = ihi > 0;
  if (any && ihi - ilo > h->max_in) return set_error(DMX_ERR_ARG, "%s: the members' padded input spans %lld bytes, more than max_in_bytes %lld", fn, (long long)(ihi - ilo), (long long)h->max_in);
  if (any && ohi - olo > h->max_out) return set_error(DMX_ERR_ARG, "%s: the members' output spans %lld bytes, more than max_out_bytes %lld", fn, (long long)(ohi - olo), (long long)h->max_out);
  for (int32_t i = 0; i < n; ++i) {
    const bool refused = (uint32_t)in_len[i] > dmxzc::kMaxIn || (uint32_t)out_len[i] > dmxzc::kMaxOut;
    s.h_desc[i] = refused ? make_uint4(0u, 0xffffffffu, 0u, 0u) : make_uint4((uint32_t)(in_off[i] - ilo), (uint32_t)in_len[i], (uint32_t)(out_off[i] - olo), (uint32_t)out_len[i]);
  }
  s.n = n; s.h2d_bytes = 0; s.d2h_bytes = 0;
  HIP_TRY(hipSetDevice(h->device));
  // From here on work is queued on the slot's stream.  If a later call fails, what is already queued may still read `in` and write
  // `out`: the stream is synchronised before the error is returned, so the caller has its buffers back either way.
  const int rc = submit_enqueue(h, s, n, in, in_off, out, out_off, out_len, any, ilo, ihi, olo, ohi);
  if (rc != DMX_OK) { (void)hipStreamSynchronize(s.stream); (void)hipGetLastError(); return rc; }
  s.busy = true;
  return DMX_OK;
}

static int submit_enqueue(dmx_inflater* h, dmx_inflater::Slot& s, int32_t n, const uint8_t* in, const int64_t* in_off, uint8_t* out, const int64_t* out_off,
                          const int32_t* out_len, bool any, int64_t ilo, int64_t ihi, int64_t olo, int64_t ohi) {
  HIP_TRY(hipEventRecord(s.ev[0], s.stream));
  if (n > 0) {
    if (any) HIP_TRY(hipMemcpyAsync(s.d_in, in + ilo, (size_t)(ihi - ilo), hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipMemcpyAsync(s.d_desc, s.h_desc, sizeof(uint4) * (size_t)n, hipMemcpyHostToDevice, s.stream));
    s.h2d_bytes = (any ? ihi - ilo : 0) + (int64_t)sizeof(uint4) * n;
  }
  HIP_TRY(hipEventRecord(s.ev[1], s.stream));
  if (n > 0) {
    hipLaunchKernelGGL(dmx_gz::k_bgzf_inflate, dim3((unsigned)n), dim3(64), 0, s.stream, s.d_in, (uint32_t)(any ? ihi - ilo : 0), s.d_out, (uint32_t)(any ? ohi - olo : 0),
                       s.d_desc, s.d_status, n);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(s.ev[2], s.stream));
  if (n > 0) {
    // the members' bytes go straight to where the caller wants them: one copy per run of members whose ranges follow one another
    int64_t run_lo = -1, run_hi = -1;
    auto flush = [&]() -> hipError_t {
      if (run_hi <= run_lo) return hipSuccess;
      s.d2h_bytes += run_hi - run_lo;
      return hipMemcpyAsync(out + run_lo, s.d_out + (run_lo - olo), (size_t)(run_hi - run_lo), hipMemcpyDeviceToHost, s.stream);
    };
    for (int32_t i = 0; i < n; ++i) {
      if (s.h_desc[i].y == 0xffffffffu || out_len[i] == 0) continue;
      if (out_off[i] != run_hi) { HIP_TRY(flush()); run_lo = out_off[i]; }
      run_hi = out_off[i] + out_len[i];
    }
    HIP_TRY(flush());
    HIP_TRY(hipMemcpyAsync(s.h_status, s.d_status, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s.stream));
    s.d2h_bytes += (int64_t)sizeof(int32_t) * n;
  }
  HIP_TRY(hipEventRecord(s.ev[3], s.stream));
  return DMX_OK;
}

extern "C" int dmx_inflater_wait(dmx_inflater* h, int32_t slot, int32_t* status, dmx_inflater_info* info) {
  const char* fn = "dmx_inflater_wait";
  if (!h) return set_error(DMX_ERR_ARG, "%s: null inflater", fn);
  if (slot < 0 || slot > 1) return set_error(DMX_ERR_ARG, "%s: slot %d is not 0 or 1", fn, slot);
  dmx_inflater::Slot& s = h->slot[slot];
  if (!s.busy) return set_error(DMX_ERR_STATE, "%s: slot %d has no batch in flight", fn, slot);
  if (s.n > 0 && !status) return set_error(DMX_ERR_ARG, "%s: null status", fn);
  HIP_TRY(hipSetDevice(h->device));
  s.busy = false;                                  // (whatever happens below, the slot is free again)
  HIP_TRY(hipStreamSynchronize(s.stream));
  int32_t ok = 0;
  for (int32_t i = 0; i < s.n; ++i) { status[i] = s.h_status[i]; ok += s.h_status[i] == 0; }
  if (info) {
    memset(info, 0, sizeof *info);
    float ms[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], s.ev[k], s.ev[k + 1]));
    info->h2d_ms = ms[0]; info->kernel_ms = ms[1]; info->d2h_ms = ms[2];
    info->h2d_bytes = s.h2d_bytes; info->d2h_bytes = s.d2h_bytes;
    info->n_members = s.n; info->n_accepted = ok; info->n_refused = s.n - ok;
  }
  return DMX_OK;
}

extern "C" int dmx_inflater_run(dmx_inflater* h, int32_t n, const uint8_t* in, const int64_t* in_off, const int32_t* in_len,
                                uint8_t* out, const int64_t* out_off, const int32_t* out_len, int32_t* status, dmx_inflater_info* info) {
  if (int rc = dmx_inflater_submit(h, 0, n, in, in_off, in_len, out, out_off, out_len)) return rc;
  return dmx_inflater_wait(h, 0, status, info);
}
