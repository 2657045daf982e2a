// cro_amd gfx950 device health probe.
//
// The MI355X-native replacement for the reference's "is the GPU alive"
// signal (forking `nvidia-smi` over pod exec, gpus.go:207-350): after the
// fabric composes a device and amdgpu binds it, this probe checks that the
// device computes and streams at the expected rates before the operator
// advertises it via CDI.  The exact check runs on ONE wave on one CU and
// the rate kernels compare nothing: every CU and SIMD is checked exactly
// only by the opt-in compute-coverage stage (coverage.hip).
//
//   1. mfma_f32_check  — one wave issues v_mfma_f32_16x16x4_f32 over a
//      K-loop; gfx950's f32-input MFMA is bitwise a k-ordered fmaf chain,
//      so the host can verify the result EXACTLY (no tolerance) — a
//      deterministic matrix-pipe + VGPR/AGPR integrity check.
//   2. bw_copy         — float4 streaming copy across a >>256-workgroup
//      grid, reporting achieved HBM3E bandwidth (expected ≈5-6.3 TB/s on a
//      healthy MI355X; gate is a loose floor).
//   3. mfma_bf16_rate  — dense v_mfma_f32_32x32x16_bf16 issue from 4
//      independent accumulators per wave; reports matrix-core TFLOP/s
//      (healthy ≈2.3-2.5 PF; loose floor gate).
//
// A call is one submission and one wait.  The check kernel's inputs and the
// expected tile never change, so the context holds them (built and uploaded
// once per device).  On the context's own non-blocking stream a call
// enqueues: a poison of the result tile, the check kernel, the copy
// launches, the rate kernel and the tile's copy into pinned host memory, with
// an event between the sections; it then waits once, on the last event, and
// compares the tile and takes both rates from event pairs.  t_mfma_ms,
// t_bw_ms and t_bf16_ms are therefore each section's device time from its
// events (with a single wait there is no host wall per section); t_setup_ms
// is the host wall up to the first enqueue.  The lengths of the two rate
// windows (copy launches, rate-kernel iterations) are the defaults below,
// set against a sweep on the device (profiles/quick_probe_windows_mi355x.md);
// cro_probe_run_windows runs the same pipeline at a caller's windows.
//
// Built with hipcc for gfx950 only (no torch dependency), with integrity.hip
// and coverage.hip, into libcroprobe.so (cro_amd/hip/build.py).  The three
// sources share their host plumbing (crohost.h) and, probe.hip and
// coverage.hip, the wave-level matrix code (cromfma.h).
//
// C ABI consumed by cro_amd/nodeops/probe.py via ctypes.  Besides the probe
// itself it has one raw entry per kernel (caller data in, raw output back)
// and a self-check of the probe's own copy launch, for the exact tests in
// tests/test_probe_quick_gpu.py.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstring>
#include <vector>

#include "crohost.h"
#include "cromfma.h"
#include "croprobe.h"

// ---------------------------------------------------------------------------
// 1. exact f32 MFMA check (v_mfma_f32_16x16x4_f32: A 16xK, B Kx16, D 16x16;
//    lane maps in cromfma.h, layouts per cdna_hip_programming.md §3)
// ---------------------------------------------------------------------------

__global__ void mfma_f32_check_kernel(const float* __restrict__ A,
                                      const float* __restrict__ B,
                                      float* __restrict__ D, int K) {
  const uint32_t lane = threadIdx.x;  // exactly one wave of 64
  const f32x4 acc = wave_mfma_f32(A, B, K, lane);
  for (int r = 0; r < 4; ++r) D[mfma_elem16(lane, r)] = acc[r];
}

// ---------------------------------------------------------------------------
// 2. HBM streaming copy
// ---------------------------------------------------------------------------

__global__ void bw_copy_kernel(const float4* __restrict__ src,
                               float4* __restrict__ dst, size_t n4) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) dst[i] = src[i];
}

// ---------------------------------------------------------------------------
// 3. bf16 MFMA issue-rate (4 independent accumulators per wave keeps the
//    32-cycle/SIMD issue pipe of v_mfma_f32_32x32x16_bf16 saturated)
// ---------------------------------------------------------------------------

// kAllLanes = false is the probe's kernel: thread 0 of each block stores its
// sum.  true stores every thread's sum (cro_probe_bf16_sink, for tests): the
// operands have the closed form A[row][k] = 0.5 + 0.0625 * ((row + k) & 7),
// B[k][col] = 0.25 + 0.03125 * ((3 * col + k) & 7) in every wave, so each
// lane's sum is known exactly.
template <bool kAllLanes>
__global__ void mfma_bf16_rate_kernel(float* __restrict__ out, int iters) {
  bf16x8 a, b;
  // non-zero, non-uniform operands: zero inputs let DVFS overclock and
  // overstate the rate (MI355X_MICROARCH.md "DVFS give-back")
  for (int i = 0; i < 8; ++i) {
    a[i] = (__bf16)(0.5f + 0.0625f * (float)((threadIdx.x + i) & 7));
    b[i] = (__bf16)(0.25f + 0.03125f * (float)((threadIdx.x * 3 + i) & 7));
  }
  f32x16 acc0 = {}, acc1 = {}, acc2 = {}, acc3 = {};
  for (int it = 0; it < iters; ++it) {
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc1, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc2, 0, 0, 0);
    acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc3, 0, 0, 0);
  }
  float s = 0.f;
  for (int i = 0; i < 16; ++i) s += acc0[i] + acc1[i] + acc2[i] + acc3[i];
  if constexpr (kAllLanes) {
    out[blockIdx.x * 256 + threadIdx.x] = s;
  } else {
    if (threadIdx.x == 0) out[blockIdx.x] = s;
  }
}

// ---------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------

// Events of one call, in stream order: around the check kernel, after the
// copy launches, after the rate kernel, after the tile's copy to the host.
enum { kEvCheck0, kEvCheck1, kEvCopies, kEvRate, kEvTile, kNumEvents };

// Per-device cached probe context (CtxBase, crohost.h): the probe runs on
// every attach, so allocations, the stream and the events are created once
// and reused, and what is the same in every call (the check kernel's inputs
// at seed 0 and the tile the host expects) is built and uploaded once — only
// the kernels, the tile's copy back and the compare run per call.
struct ProbeCtx : CtxBase {
  long long vram_total = 0, vram_free = 0;  // hipMemGetInfo is sysfs-backed
                                            // and ms-scale: snapshot at init
  float *dA = nullptr, *dB = nullptr, *dD = nullptr;
  float4 *src = nullptr, *dst = nullptr;
  float* sink = nullptr;
  hipStream_t stream = nullptr;  // hipStreamNonBlocking: a probe neither waits
                                 // for nor holds up the process's other streams
  hipEvent_t ev[kNumEvents] = {};
  float* hD = nullptr;                  // pinned: dD lands here in-stream
  float refD[CRO_COV_F32_ELEMS] = {0};  // expected tile; calls compare, never write
  char gcn_arch[64] = {0};  // hipGetDeviceProperties costs milliseconds —
                            // queried once, the probe runs per attach
};
static ProbeCtx g_ctx[kMaxDevices];

constexpr int kBwGrid = 8192;
constexpr size_t kBwBytes = (size_t)256 << 20;  // each of src and dst
constexpr int kGuardVecs = 64;  // cro_probe_copy: vectors after dst, preset to 0xA5
constexpr unsigned long long kMaxCopyVecs = kBwBytes / sizeof(float4);
constexpr int kMaxCopyGrid = 1 << 16;
constexpr int kMaxSinkBlocks = 1024;
constexpr int kMaxSinkIters = 1 << 16;
constexpr int kRateBlocks = 1024;  // of 256 threads: 4 waves per SIMD on 256 CUs
// The two rate windows (struct CroProbeWindows: 0 takes these), and the
// largest a caller may ask for.  Each default is the shortest of the swept
// windows (1, 2, 4, 8 launches; 256 to 2048 iterations) whose every reading,
// back to back and from an idle device, stayed within the band the longest
// one spans in the same run (profiles/quick_probe_windows_mi355x.md): 8
// launches ≈0.80 ms (4 launches read up to 3 % low from idle), 1024
// iterations ≈0.25-0.28 ms (512 read 4 % low from idle).
constexpr int kDefaultCopyLaunches = 8;
constexpr int kDefaultBf16Iters = 1024;
constexpr int kMaxCopyLaunches = 64;
constexpr int kMaxBf16Iters = 1 << 16;

static void launch_copy(const float4* src, float4* dst, size_t n4, int grid_blocks,
                        hipStream_t stream = nullptr) {
  hipLaunchKernelGGL(bw_copy_kernel, dim3(grid_blocks), dim3(kBlock), 0, stream, src, dst, n4);
}

// The probe's own copy, on the context's stream: the launch whose bytes
// hbm_gbps is credited for.
static void launch_probe_copy(const ProbeCtx* ctx) {
  launch_copy(ctx->src, ctx->dst, kBwBytes / sizeof(float4), kBwGrid, ctx->stream);
}

static void launch_probe_check(const ProbeCtx* ctx) {
  hipLaunchKernelGGL(mfma_f32_check_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->dA, ctx->dB,
                     ctx->dD, CRO_COV_F32_K);
}

static void launch_probe_rate(const ProbeCtx* ctx, int iters) {
  hipLaunchKernelGGL(mfma_bf16_rate_kernel<false>, dim3(kRateBlocks), dim3(256), 0, ctx->stream,
                     ctx->sink, iters);
}

// Caller holds ctx->mu and has made `device` current.
static hipError_t ensure_ctx(ProbeCtx* ctx, int device) {
  if (ctx->ready) return hipSuccess;
  TRY(hipMalloc(&ctx->dA, 16 * CRO_COV_F32_K * sizeof(float)));
  TRY(hipMalloc(&ctx->dB, CRO_COV_F32_K * 16 * sizeof(float)));
  TRY(hipMalloc(&ctx->dD, CRO_COV_F32_ELEMS * sizeof(float)));
  TRY(hipMalloc(&ctx->src, kBwBytes));
  TRY(hipMalloc(&ctx->dst, kBwBytes));
  TRY(hipMemset(ctx->src, 0x5a, kBwBytes));
  TRY(hipMalloc(&ctx->sink, kRateBlocks * sizeof(float)));
  TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  for (hipEvent_t& e : ctx->ev) TRY(hipEventCreate(&e));
  TRY(hipHostMalloc(&ctx->hD, sizeof(ctx->refD), hipHostMallocDefault));
  // inputs and expected tile are the coverage stage's at seed 0
  // (crocoverage.h), the same for every call on every device
  float hA[16 * CRO_COV_F32_K], hB[CRO_COV_F32_K * 16];
  cro_cov_make_f32(0, hA, hB);
  cro_cov_ref_f32(hA, hB, ctx->refD);
  TRY(hipMemcpy(ctx->dA, hA, sizeof(hA), hipMemcpyHostToDevice));
  TRY(hipMemcpy(ctx->dB, hB, sizeof(hB), hipMemcpyHostToDevice));
  hipDeviceProp_t prop;
  TRY(hipGetDeviceProperties(&prop, device));
  snprintf(ctx->gcn_arch, sizeof(ctx->gcn_arch), "%s", prop.gcnArchName);
  size_t free_b = 0, total_b = 0;
  TRY(hipMemGetInfo(&free_b, &total_b));
  ctx->vram_total = (long long)total_b;
  ctx->vram_free = (long long)free_b;
  // one warm round at init covers kernel-code upload (the fill kernel behind
  // hipMemsetAsync included); per-call warms are off the attach path.  The
  // set-up above went through the null stream, which this stream does not
  // wait for: it is drained before the stream sees its first command.
  TRY(hipDeviceSynchronize());
  TRY(hipMemsetAsync(ctx->dD, 0xFF, sizeof(ctx->refD), ctx->stream));
  launch_probe_check(ctx);
  launch_probe_copy(ctx);
  launch_probe_rate(ctx, 64);
  TRY(hipGetLastError());
  TRY(hipMemcpyAsync(ctx->hD, ctx->dD, sizeof(ctx->refD), hipMemcpyDeviceToHost, ctx->stream));
  TRY(hipStreamSynchronize(ctx->stream));
  ctx->ready = 1;
  return hipSuccess;
}

// Inside enqueue_and_wait: a HIP error goes back to the caller, with the
// failing call's text in *what for the message.
#define STEP(expr)                \
  do {                            \
    hipError_t _e = (expr);       \
    if (_e != hipSuccess) {       \
      *what = #expr;              \
      return _e;                  \
    }                             \
  } while (0)

// One call's whole submission on the context's stream, then its one wait.
// *enqueued tells the caller that the stream may hold work of this call.
static hipError_t enqueue_and_wait(ProbeCtx* ctx, int copy_launches, int bf16_iters,
                                   bool skip_check, bool* enqueued, const char** what) {
  hipStream_t st = ctx->stream;
  *enqueued = true;
  // poison first: a check kernel that did not run must not pass on the tile
  // the call before left in dD
  STEP(hipMemsetAsync(ctx->dD, 0xFF, sizeof(ctx->refD), st));
  STEP(hipEventRecord(ctx->ev[kEvCheck0], st));
  if (!skip_check) launch_probe_check(ctx);
  STEP(hipGetLastError());
  STEP(hipEventRecord(ctx->ev[kEvCheck1], st));
  for (int i = 0; i < copy_launches; ++i) launch_probe_copy(ctx);
  STEP(hipGetLastError());
  STEP(hipEventRecord(ctx->ev[kEvCopies], st));
  launch_probe_rate(ctx, bf16_iters);
  STEP(hipGetLastError());
  STEP(hipEventRecord(ctx->ev[kEvRate], st));
  STEP(hipMemcpyAsync(ctx->hD, ctx->dD, sizeof(ctx->refD), hipMemcpyDeviceToHost, st));
  STEP(hipEventRecord(ctx->ev[kEvTile], st));
  STEP(hipEventSynchronize(ctx->ev[kEvTile]));
  return hipSuccess;
}

#undef STEP

// The probe at given windows.  `o` and the windows are validated by the two
// entries below; t0 is the host clock at the entry.
static int run_pipeline(int device, const struct CroProbeOpts& o, int copy_launches,
                        int bf16_iters, bool skip_check, struct CroProbeResult* out, double t0) {
  const double hbm_floor = o.hbm_floor_gbps > 0.0 ? o.hbm_floor_gbps : 500.0;
  const double bf16_floor = o.bf16_floor_tflops > 0.0 ? o.bf16_floor_tflops : 100.0;

  std::unique_lock<std::mutex> lock;
  ProbeCtx* ctx = enter_device(g_ctx, device, lock, out->msg, sizeof(out->msg));
  if (ctx == nullptr) return -1;
  CHECK(ensure_ctx(ctx, device));
  snprintf(out->gcn_arch, sizeof(out->gcn_arch), "%s", ctx->gcn_arch);
  out->vram_total = ctx->vram_total;
  out->vram_free = ctx->vram_free;
  out->t_setup_ms = now_ms() - t0;

  bool enqueued = false;
  const char* what = "";
  const hipError_t e = enqueue_and_wait(ctx, copy_launches, bf16_iters, skip_check, &enqueued,
                                        &what);
  if (e != hipSuccess) {
    // the next caller must find neither the events nor the pinned tile in
    // flight: drain what was enqueued before the slot's mutex is released
    if (enqueued) (void)hipStreamSynchronize(ctx->stream);
    snprintf(out->msg, sizeof(out->msg), "%s failed: %s", what, hipGetErrorString(e));
    return -1;
  }

  // -- exact f32 MFMA ------------------------------------------------------
  const float* want = ctx->refD;
  float flipped[CRO_COV_F32_ELEMS];
  if (o.selftest_mode == 1) {
    // self-test, for tests only: one bit of one expected element is flipped,
    // so the exact gate must fire on data alone (as coverage.hip's mode 1).
    // The flip is made in this call's copy; the cached tile stays as it is.
    memcpy(flipped, ctx->refD, sizeof(flipped));
    uint32_t u;
    memcpy(&u, &flipped[o.selftest_elem], sizeof(u));
    u ^= 1u << o.selftest_bit;
    memcpy(&flipped[o.selftest_elem], &u, sizeof(u));
    want = flipped;
  }
  out->mfma_f32_exact = (memcmp(ctx->hD, want, sizeof(flipped)) == 0) ? 1 : 0;

  float ms = 0.f;
  CHECK(hipEventElapsedTime(&ms, ctx->ev[kEvCheck0], ctx->ev[kEvCheck1]));
  out->t_mfma_ms = ms;
  // -- HBM bandwidth -------------------------------------------------------
  // 256 MiB src + dst from the cached context (512 MiB of traffic per launch,
  // copy_launches of them per measurement — ample signal without putting
  // hipMalloc on the attach-latency path or pinning more of the 288 GB than a
  // gate needs)
  CHECK(hipEventElapsedTime(&ms, ctx->ev[kEvCheck1], ctx->ev[kEvCopies]));
  out->hbm_gbps = (double)(2.0 * kBwBytes * copy_launches) / (ms * 1e6);
  out->t_bw_ms = ms;
  // -- bf16 MFMA rate ------------------------------------------------------
  CHECK(hipEventElapsedTime(&ms, ctx->ev[kEvCopies], ctx->ev[kEvRate]));
  double waves = (double)kRateBlocks * 256.0 / 64.0;
  double flops = waves * 4.0 * (double)bf16_iters * 2.0 * 32.0 * 32.0 * 16.0;
  out->bf16_tflops = flops / (ms * 1e9);
  out->t_bf16_ms = ms;

  // gates: exact MFMA is hard; bandwidth/rate are loose floors so a busy or
  // power-capped chip never false-fails
  if (!out->mfma_f32_exact) {
    snprintf(out->msg, sizeof(out->msg), "f32 MFMA mismatch vs host fmaf chain");
    return -2;
  }
  if (out->hbm_gbps < hbm_floor) {
    snprintf(out->msg, sizeof(out->msg), "HBM bandwidth %.0f GB/s below floor", out->hbm_gbps);
    return -3;
  }
  if (out->bf16_tflops < bf16_floor) {
    snprintf(out->msg, sizeof(out->msg), "bf16 MFMA %.0f TF below floor", out->bf16_tflops);
    return -4;
  }
  out->ok = 1;
  snprintf(out->msg, sizeof(out->msg), "ok");
  return 0;
}

extern "C" int cro_probe_run_opts(int device, const struct CroProbeOpts* opts,
                                  struct CroProbeResult* out) {
  memset(out, 0, sizeof(*out));
  out->ok = 0;
  const double t0 = now_ms();

  struct CroProbeOpts o;
  memset(&o, 0, sizeof(o));
  if (opts) o = *opts;
  // !(x >= 0) also refuses a NaN
  if (!(o.hbm_floor_gbps >= 0.0)) return bad_arg(out, "hbm_floor_gbps");
  if (!(o.bf16_floor_tflops >= 0.0)) return bad_arg(out, "bf16_floor_tflops");
  if (o.selftest_mode < 0 || o.selftest_mode > 1) return bad_arg(out, "selftest_mode");
  if (o.selftest_bit < 0 || o.selftest_bit > 31) return bad_arg(out, "selftest_bit");
  if (o.selftest_elem >= CRO_COV_F32_ELEMS) return bad_arg(out, "selftest_elem");
  return run_pipeline(device, o, kDefaultCopyLaunches, kDefaultBf16Iters, false, out, t0);
}

// The same pipeline with the caller's rate windows and the floors at their
// defaults: how the default windows were chosen
// (profiles/quick_probe_windows_mi355x.md), and a seam for tests.
extern "C" int cro_probe_run_windows(int device, const struct CroProbeWindows* w,
                                     struct CroProbeResult* out) {
  memset(out, 0, sizeof(*out));
  out->ok = 0;
  const double t0 = now_ms();

  struct CroProbeWindows win;
  memset(&win, 0, sizeof(win));
  if (w) win = *w;
  if (win.copy_launches < 0 || win.copy_launches > kMaxCopyLaunches)
    return bad_arg(out, "copy_launches");
  if (win.bf16_iters < 0 || win.bf16_iters > kMaxBf16Iters) return bad_arg(out, "bf16_iters");
  if (win.skip_check_launch < 0 || win.skip_check_launch > 1)
    return bad_arg(out, "skip_check_launch");
  if (win.reserved < 0) return bad_arg(out, "reserved");
  struct CroProbeOpts o;
  memset(&o, 0, sizeof(o));
  return run_pipeline(device, o, win.copy_launches ? win.copy_launches : kDefaultCopyLaunches,
                      win.bf16_iters ? win.bf16_iters : kDefaultBf16Iters,
                      win.skip_check_launch == 1, out, t0);
}

extern "C" int cro_probe_run(int device, struct CroProbeResult* out) {
  return cro_probe_run_opts(device, nullptr, out);
}

// ---------------------------------------------------------------------------
// raw entries for tests: each kernel of the probe on caller data
// ---------------------------------------------------------------------------

// Raw MFMA tile entry for numerics tests: D(16x16) = A(16xK) @ B(Kx16) on
// the f32 matrix pipe; compared bit for bit against the k-ordered fmaf chain
// in tests/test_probe_quick_gpu.py.  K a multiple of 4, at most 4096.
extern "C" int cro_probe_mfma_f32(int device, const float* A, const float* B,
                                  float* D, int K) {
  if (A == nullptr || B == nullptr || D == nullptr) return -10;
  if (K <= 0 || K > kMaxTileK || (K & 3) != 0) return -10;
  const size_t in_bytes = (size_t)16 * K * sizeof(float), out_bytes = 256 * sizeof(float);
  if (hipSetDevice(device) != hipSuccess) return -1;
  DevBuf<float> dA, dB, dD;
  const auto run = [&]() -> hipError_t {
    TRY(dA.alloc(in_bytes));
    TRY(dB.alloc(in_bytes));
    TRY(dD.alloc(out_bytes));
    TRY(hipMemcpy(dA.get(), A, in_bytes, hipMemcpyHostToDevice));
    TRY(hipMemcpy(dB.get(), B, in_bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(mfma_f32_check_kernel, dim3(1), dim3(64), 0, 0, dA.get(), dB.get(),
                       dD.get(), K);
    TRY(hipGetLastError());
    return hipMemcpy(D, dD.get(), out_bytes, hipMemcpyDeviceToHost);
  };
  return run() == hipSuccess ? 0 : -1;
}

// bw_copy_kernel on caller data: n4 16-byte vectors, grid_blocks x 256
// threads.  dst is followed by 64 guard vectors preset to 0xA5 (as the whole
// of dst is, so a vector the kernel skipped shows); *guard_ok tells whether
// they came back untouched.  Returns 0, -10 for a bad argument, -1 for a HIP
// error and -11 when the kernel changed src.
extern "C" int cro_probe_copy(int device, const void* src_host, unsigned long long n4,
                              int grid_blocks, void* dst_host, int* guard_ok) {
  if (src_host == nullptr || dst_host == nullptr || guard_ok == nullptr) return -10;
  if (n4 == 0 || n4 > kMaxCopyVecs) return -10;
  if (grid_blocks < 1 || grid_blocks > kMaxCopyGrid) return -10;
  *guard_ok = 0;
  const size_t bytes = (size_t)n4 * sizeof(float4);
  const size_t guard_bytes = kGuardVecs * sizeof(float4);
  if (hipSetDevice(device) != hipSuccess) return -1;
  DevBuf<float4> src, dst;
  std::vector<unsigned char> back(bytes > guard_bytes ? bytes : guard_bytes);
  const auto run = [&]() -> hipError_t {
    TRY(src.alloc(bytes));
    TRY(dst.alloc(bytes + guard_bytes));
    TRY(hipMemcpy(src.get(), src_host, bytes, hipMemcpyHostToDevice));
    TRY(hipMemset(dst.get(), 0xA5, bytes + guard_bytes));
    launch_copy(src.get(), dst.get(), (size_t)n4, grid_blocks);
    TRY(hipGetLastError());
    TRY(hipMemcpy(dst_host, dst.get(), bytes, hipMemcpyDeviceToHost));
    TRY(hipMemcpy(back.data(), dst.get() + n4, guard_bytes, hipMemcpyDeviceToHost));
    int ok = 1;
    for (size_t i = 0; i < guard_bytes; ++i) ok &= back[i] == 0xA5;
    *guard_ok = ok;
    return hipMemcpy(back.data(), src.get(), bytes, hipMemcpyDeviceToHost);
  };
  if (run() != hipSuccess) return -1;
  return memcmp(back.data(), src_host, bytes) == 0 ? 0 : -11;
}

// The probe's own copy launch, once, on the cached context with dst zeroed
// first: *n_bad counts the bytes of dst that are not src's 0x5a afterwards,
// *first_bad is the lowest such byte offset (~0 when none).  Shows that the
// grid and size hbm_gbps is credited for write every byte of dst.
extern "C" int cro_probe_bw_selfcheck(int device, unsigned long long* n_bad,
                                      unsigned long long* first_bad) {
  if (n_bad == nullptr || first_bad == nullptr) return -10;
  *n_bad = 0;
  *first_bad = ~0ull;
  std::unique_lock<std::mutex> lock;
  ProbeCtx* ctx = enter_device(g_ctx, device, lock, nullptr, 0);  // rc only, no message
  if (ctx == nullptr) return -1;
  const auto copy_once = [&]() -> hipError_t {
    TRY(ensure_ctx(ctx, device));
    TRY(hipMemsetAsync(ctx->dst, 0, kBwBytes, ctx->stream));
    launch_probe_copy(ctx);
    TRY(hipGetLastError());
    return hipSuccess;
  };
  // whatever was enqueued is drained before dst is read or the mutex released
  const hipError_t enq = copy_once();
  const hipError_t done = ctx->stream ? hipStreamSynchronize(ctx->stream) : hipSuccess;
  if (enq != hipSuccess || done != hipSuccess) return -1;
  const size_t chunk = (size_t)32 << 20;
  std::vector<unsigned char> host(chunk);
  for (size_t off = 0; off < kBwBytes; off += chunk) {
    if (hipMemcpy(host.data(), (const unsigned char*)ctx->dst + off, chunk,
                  hipMemcpyDeviceToHost) != hipSuccess)
      return -1;
    for (size_t i = 0; i < chunk; i += 8) {
      unsigned long long w;
      memcpy(&w, &host[i], 8);
      if (w == 0x5a5a5a5a5a5a5a5aull) continue;
      for (size_t j = i; j < i + 8; ++j) {
        if (host[j] == 0x5a) continue;
        if (*n_bad == 0) *first_bad = off + j;
        ++*n_bad;
      }
    }
  }
  return 0;
}

// mfma_bf16_rate_kernel on `blocks` x 256 threads for `iters` iterations.
// all_lanes = 0: the probe's kernel, out_host gets `blocks` floats (thread 0
// of each block); else every thread's sum, blocks * 256 floats.  The device
// buffer is preset to 0xFF, so a value the kernel did not store reads as NaN.
extern "C" int cro_probe_bf16_sink(int device, int blocks, int iters, int all_lanes,
                                   float* out_host) {
  if (out_host == nullptr) return -10;
  if (blocks < 1 || blocks > kMaxSinkBlocks) return -10;
  if (iters < 0 || iters > kMaxSinkIters) return -10;
  const size_t bytes = (size_t)blocks * (all_lanes ? kBlock : 1) * sizeof(float);
  if (hipSetDevice(device) != hipSuccess) return -1;
  DevBuf<float> d;
  const auto run = [&]() -> hipError_t {
    TRY(d.alloc(bytes));
    TRY(hipMemset(d.get(), 0xFF, bytes));
    if (all_lanes)
      hipLaunchKernelGGL(mfma_bf16_rate_kernel<true>, dim3(blocks), dim3(kBlock), 0, 0, d.get(),
                         iters);
    else
      hipLaunchKernelGGL(mfma_bf16_rate_kernel<false>, dim3(blocks), dim3(kBlock), 0, 0, d.get(),
                         iters);
    TRY(hipGetLastError());
    return hipMemcpy(out_host, d.get(), bytes, hipMemcpyDeviceToHost);
  };
  return run() == hipSuccess ? 0 : -1;
}

// Raw VRAM alloc/free for the self-identification fingerprint
// (cro_amd/nodeops/kfd.py resolve_self_kfd_pid): the operator finds its own
// host pid in /sys/class/kfd/kfd/proc by watching which vram_<gpu_id> file
// grows by a marker-sized hipMalloc.
extern "C" void* cro_probe_alloc(int device, long long bytes) {
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  void* p = nullptr;
  if (hipMalloc(&p, (size_t)bytes) != hipSuccess) return nullptr;
  if (hipMemset(p, 1, (size_t)bytes) != hipSuccess) { (void)hipFree(p); return nullptr; }
  if (hipDeviceSynchronize() != hipSuccess) { (void)hipFree(p); return nullptr; }
  return p;
}

extern "C" void cro_probe_free(void* p) { (void)hipFree(p); }

extern "C" int cro_probe_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return -1;
  return count;
}

extern "C" int cro_probe_pci_bus_id(int device, char* buf, int len) {
  if (hipDeviceGetPCIBusId(buf, len, device) != hipSuccess) return -1;
  return 0;
}
