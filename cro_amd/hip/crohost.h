// Host plumbing shared by every stage's .hip source, in libcroprobe.so and in
// the stage libraries of their own: error macros, bounds, the per-device
// context base and its entry, event-timed launches, an owning device buffer,
// and for the stages that write one record per wave (coverage.hip,
// formats.hip, movement.hip) the record buffer and the round driver.
//
// Internal and HIP-only: the C ABI headers (croprobe.h, crocoverage.h,
// cropattern.h and the stages' own) never include it, so a host compiler
// without HIP can still include those.  Everything here has internal linkage;
// no library exports anything from this file.
#pragma once

#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

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

// -- the stages with one record per wave --------------------------------------
// One workgroup per CU, one record per wave and round; the host relaunches
// until every CU and SIMD was seen or a wave was bad.  A stage keeps its option
// checks, its kernel parameters, its launch and its mismatch message; the rest
// is here.  Result is the stage's Cro*Result: ok, rounds, agg, first_bad_round,
// first_bad_record, gpu_ms and msg are what these templates touch.

// The device record buffer of a cached context: grows on demand, lives as long
// as the process.
template <class Record>
struct RecordBuf {
  Record* d = nullptr;
  size_t cap = 0;

  // Holds at least n records afterwards.
  hipError_t reserve(size_t n) {
    if (cap >= n) return hipSuccess;
    if (d) (void)hipFree(d);
    d = nullptr;
    cap = 0;
    TRY(hipMalloc(&d, n * sizeof(Record)));
    cap = n;
    return hipSuccess;
  }
};

// What an entry point hands its run function: all zero, no bad wave.
// `aggregate` is the stage's cro_*_aggregate(records, n, &agg), which over no
// records leaves the cleared aggregate.
template <class Result, class Aggregate>
void clear_result(Result* out, Aggregate&& aggregate) {
  memset(out, 0, sizeof(*out));
  out->first_bad_round = out->first_bad_record = -1;
  aggregate(nullptr, 0, &out->agg);
}

// The rounds of one run on `d_records`, which holds per_round * max_rounds
// records.  `launch(d_round)` enqueues one round's kernel(s), which write the
// per_round records at d_round.  Per run one memset of the buffer; per round
// one timed window and one copy back.  Stops after the round in which a wave
// was bad, the device was covered (`cus` CUs, four SIMDs each) or max_rounds
// was reached, then fills rounds, gpu_ms, agg and, where a wave was bad, where
// the first one is; at most max_records records go to records_out, round-major.
// 0, or -1 with the reason in msg: a HIP error or a wave that did not report.
template <class Record, class Result, class Launch, class Aggregate>
int run_rounds(const CtxBase& ctx, Record* d_records, int cus, size_t per_round, int max_rounds,
               Launch&& launch, Aggregate&& aggregate, Result* out, Record* records_out,
               int max_records) {
  const size_t n_max = per_round * (size_t)max_rounds;
  std::vector<Record> records(n_max);
  CHECK(hipMemset(d_records, 0, n_max * sizeof(Record)));
  int rounds = 0;
  double gpu_ms = 0.0;
  for (;;) {
    Record* d_round = d_records + (size_t)rounds * per_round;
    float ms = 0.f;
    CHECK(timed_ms(ctx, &ms, [&] { launch(d_round); }));
    gpu_ms += ms;
    CHECK(hipMemcpy(records.data() + (size_t)rounds * per_round, d_round,
                     per_round * sizeof(Record), hipMemcpyDeviceToHost));
    ++rounds;
    aggregate(records.data(), (size_t)rounds * per_round, &out->agg);
    const bool covered = out->agg.cus_seen >= cus && out->agg.simds_seen >= 4 * out->agg.cus_seen;
    if (out->agg.waves_bad || covered || rounds >= max_rounds) break;
  }
  out->rounds = rounds;
  out->gpu_ms = gpu_ms;
  const size_t n = (size_t)rounds * per_round;
  if (records_out && max_records > 0) {
    const size_t m = n < (size_t)max_records ? n : (size_t)max_records;
    memcpy(records_out, records.data(), m * sizeof(Record));
  }
  if (out->agg.waves_run != n) {
    // a wave that never wrote its record: the launch did not run to the end
    snprintf(out->msg, sizeof(out->msg), "%llu of %zu waves reported", out->agg.waves_run, n);
    return -1;
  }
  if (out->agg.waves_bad) {
    out->first_bad_round = (int)((size_t)out->agg.first_bad_index / per_round);
    out->first_bad_record = (int)((size_t)out->agg.first_bad_index % per_round);
  }
  return 0;
}

// How a run without a bad wave ends: `rc` where fewer CUs were seen than the
// floor asks for, else ok.
template <class Result>
int coverage_floor(Result* out, int cus, double min_cu_fraction, int rc) {
  if (min_cu_fraction > 0.0 && (double)out->agg.cus_seen < min_cu_fraction * (double)cus) {
    snprintf(out->msg, sizeof(out->msg),
             "coverage %d of %d CUs after %d rounds is below the floor %.3f", out->agg.cus_seen,
             cus, out->rounds, min_cu_fraction);
    return rc;
  }
  out->ok = 1;
  snprintf(out->msg, sizeof(out->msg), "ok");
  return 0;
}

}  // namespace
