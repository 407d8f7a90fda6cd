// Owners of what the engine holds on the device: buffers, events, streams and pinned host memory.  Each frees in its destructor, so
// an engine (or a call's temporaries) goes away by going out of scope, whichever return leaves the function.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "dmx_internal.hpp"

#define HIP_TRY(expr)                                                                                               \
  do {                                                                                                              \
    hipError_t _e = (expr);                                                                                         \
    if (_e != hipSuccess) return dmx::set_error(DMX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                                __FILE__, __LINE__);                                                \
  } while (0)

namespace dmx {

// A device buffer and its capacity in bytes.  Converts to its pointer, so it is passed to kernels and copies like one.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  // At least `bytes`, kept across calls.  hipFree waits for the whole device, so a job whose ranges alternate between two engines
  // must not free and allocate per range: buffers only grow (with some slack for the next, slightly larger range).
  int ensure(size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    if (p_ && cap_ >= bytes) return DMX_OK;
    return alloc(bytes + bytes / 16);
  }
  // A fresh buffer of exactly `bytes` (tables and matrices of a fixed size); what it held is freed first.
  int alloc(size_t bytes) {
    reset();
    HIP_TRY(hipMalloc((void**)&p_, bytes));
    cap_ = bytes;
    return DMX_OK;
  }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr; cap_ = 0;
  }
  T* get() const { return p_; }
  size_t cap() const { return cap_; }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// An event, created by create() or by the first record().  Converts to its handle.
class Event {
 public:
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { if (ev_) (void)hipEventDestroy(ev_); }
  int create(unsigned flags = hipEventDefault) {
    if (!ev_) HIP_TRY(hipEventCreateWithFlags(&ev_, flags));
    return DMX_OK;
  }
  int record(hipStream_t s) {
    if (int rc = create()) return rc;
    HIP_TRY(hipEventRecord(ev_, s));
    return DMX_OK;
  }
  operator hipEvent_t() const { return ev_; }

 private:
  hipEvent_t ev_ = nullptr;
};

// The two events that bracket a feature's device work on the engine's stream.
struct EventPair {
  Event start, stop;
  int record_start(hipStream_t s) {
    if (int rc = stop.create()) return rc;
    return start.record(s);
  }
  int record_stop(hipStream_t s) { return stop.record(s); }
  int elapsed_ms(float* ms) const {     // (both recorded, and the stream synchronised since)
    HIP_TRY(hipEventElapsedTime(ms, start, stop));
    return DMX_OK;
  }
};

class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { if (s_) (void)hipStreamDestroy(s_); }
  int create(unsigned flags) {
    HIP_TRY(hipStreamCreateWithFlags(&s_, flags));
    return DMX_OK;
  }
  int create(unsigned flags, int priority) {
    HIP_TRY(hipStreamCreateWithPriority(&s_, flags, priority));
    return DMX_OK;
  }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

// Pinned host memory.
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { if (p_) (void)hipHostFree(p_); }
  int ensure(size_t bytes) {             // (one size per buffer: allocated once)
    if (!p_) HIP_TRY(hipHostMalloc(&p_, bytes, hipHostMallocDefault));
    return DMX_OK;
  }
  void* get() const { return p_; }

 private:
  void* p_ = nullptr;
};

}  // namespace dmx
