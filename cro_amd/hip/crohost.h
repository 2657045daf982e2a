// Host plumbing shared by the stages of libcroprobe.so (probe.hip,
// integrity.hip, coverage.hip): error macro, bounds, the per-device context
// base and its entry, event-timed launches and an owning device buffer.
//
// Internal and HIP-only: the C ABI headers (croprobe.h, crocoverage.h,
// cropattern.h) never include it, so a host compiler without HIP can still
// include those.  Everything here has internal linkage; the library exports
// nothing from this file.
#pragma once

#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <mutex>

namespace {

constexpr int kMaxDevices = 64;  // device ordinals a stage caches a context for
constexpr int kBlock = 256;
constexpr int kMaxTileK = 4096;  // raw tile entries: largest K

inline double now_ms() {
  return std::chrono::duration<double, std::milli>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

// For functions that return the stage's rc and have the result struct at
// `out`: a HIP error is rc -1 with the failing call in out->msg.
#define CHECK(expr)                                                          \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      snprintf(out->msg, sizeof(out->msg), "%s failed: %s", #expr,           \
               hipGetErrorString(_e));                                       \
      out->ok = 0;                                                           \
      return -1;                                                             \
    }                                                                        \
  } while (0)

// For helpers that hand the HIP error on to such a caller.
#define TRY(expr)                                                            \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) return _e;                                         \
  } while (0)

template <class Result>
int bad_arg(Result* out, const char* what) {
  snprintf(out->msg, sizeof(out->msg), "bad argument: %s", what);
  out->ok = 0;
  return -1;
}

// What every stage's per-device cached context starts with.  Each stage keeps
// an array of its own, so the stages can run at the same time on one device;
// the mutex serialises concurrent reconcile workers within one stage: without
// it two first calls both allocate, and any two calls share e0/e1.
struct CtxBase {
  std::mutex mu;
  int ready = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
};

// Entry of a stage: validates the ordinal, locks the device's slot of the
// stage's own array and makes the device current.  Returns null with the
// reason in msg (msg_len 0: nobody reads it); `lock` is held on success.
template <class Ctx>
Ctx* enter_device(Ctx (&slots)[kMaxDevices], int device, std::unique_lock<std::mutex>& lock,
                  char* msg, size_t msg_len) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess) {
    snprintf(msg, msg_len, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
    return nullptr;
  }
  if (device < 0 || device >= count) {
    snprintf(msg, msg_len, "device %d out of range (%d present)", device, count);
    return nullptr;
  }
  if (device >= kMaxDevices) {
    snprintf(msg, msg_len, "device ordinal %d above cache limit", device);
    return nullptr;
  }
  lock = std::unique_lock<std::mutex>(slots[device].mu);
  e = hipSetDevice(device);
  if (e != hipSuccess) {
    snprintf(msg, msg_len, "hipSetDevice failed: %s", hipGetErrorString(e));
    return nullptr;
  }
  return &slots[device];
}

// One event-timed window on the context's events: whatever `enqueue` puts on
// the stream (one launch, several, or a copy), then one synchronise.  A
// failed launch or copy inside `enqueue` is what hipGetLastError reports.
template <class Enqueue>
hipError_t timed_ms(const CtxBase& ctx, float* ms, Enqueue&& enqueue) {
  TRY(hipEventRecord(ctx.e0));
  enqueue();
  TRY(hipGetLastError());
  TRY(hipEventRecord(ctx.e1));
  TRY(hipEventSynchronize(ctx.e1));
  return hipEventElapsedTime(ms, ctx.e0, ctx.e1);
}

// Device memory held by one call and released on every way out.  (The cached
// contexts keep plain pointers: those live as long as the process.)
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { (void)free(); }

  hipError_t alloc(size_t bytes) { return hipMalloc(&p_, bytes); }
  hipError_t free() {
    T* p = p_;
    p_ = nullptr;
    return p ? hipFree(p) : hipSuccess;
  }
  T* get() const { return p_; }

 private:
  T* p_ = nullptr;
};

}  // namespace
