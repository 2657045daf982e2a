// cro_amd gfx950 deep probe: data integrity of VRAM and of the host link.
//
// The quick probe (probe.hip) gates on the matrix pipe and on rates; it
// never looks at a byte that went through HBM or across the fabric link.
// This stage does, with an address-dependent pattern (cropattern.h):
//
//   vram        — fill every chunk of the span, then verify every chunk
//                 (all resident, so aliasing between chunks shows), for
//                 the pattern and for its complement.
//   h2d_dma     — host writes a pinned buffer → hipMemcpy → device verifies.
//   d2h_dma     — device fills → hipMemcpy → host verifies.
//   h2d_kernel  — the verify kernel reads the pinned buffer across the link.
//   d2h_kernel  — the fill kernel writes the pinned buffer across the link.
//
// The same two kernels serve VRAM pointers and device-mapped pinned host
// pointers.  Gates are on data (any mismatch or HIP error fails); rates are
// reported, and gated only by the optional link_floor_gbps.
//
// Everything of this stage that needs no HIP (the host side of the link
// stages, the sizes, the chunk plan, each stage's seed and polarity) is in
// crointegrity.h, which the CPU tests compile on their own.
//
// Compiled with probe.hip and coverage.hip into libcroprobe.so
// (cro_amd/hip/build.py); host plumbing shared with them in crohost.h.

#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>

#include "crohost.h"
#include "crointegrity.h"
#include "cropattern.h"
#include "croprobe.h"

namespace {

using namespace crointegrity;  // PatternReport, host side, sizes, plan, stages

// 1024 workgroups x 256 lanes x 16 B = 4 MiB (2^18 vectors) per grid pass:
// 4 workgroups on each of the 256 CUs, grid-stride for the rest.
constexpr unsigned kMaxGrid = 1024;

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void pattern_fill_kernel(
    uint32_t* __restrict__ dst, uint64_t n_words, uint64_t base_word, uint32_t seed,
    uint32_t invert) {
  const uint64_t n4 = n_words >> 2;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst);
  for (uint64_t i = tid; i < n4; i += stride) {
    d4[i] = cro_pattern_vec4(base_word + (i << 2), seed, invert);
  }
  const uint64_t tail0 = n4 << 2;  // n_words % 4 trailing words, one lane each
  if (tid < n_words - tail0)
    dst[tail0 + tid] = cro_pattern_word(base_word + tail0 + tid, seed, invert);
}

// Mismatches are counted per wave before anything touches global memory:
// each compare is balloted across the 64 lanes and the 64-bit mask is
// popcounted (__popcll — a 32-bit popcount would drop lanes 32-63).  The
// loop runs on the vector index of lane 0, which every lane of a wave
// shares, so all 64 lanes reach every ballot and the counters are
// wave-uniform.  A wave that saw nothing bad issues no atomic at all; one
// that did issues one add, one min and one or.
__global__ __launch_bounds__(kBlock) void pattern_verify_kernel(
    const uint32_t* __restrict__ src, uint64_t n_words, uint64_t base_word,
    uint32_t seed, uint32_t invert, PatternReport* __restrict__ report) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t n4 = n_words >> 2;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(src);

  unsigned long long wave_bad = 0;
  unsigned long long wave_first = ~0ull;
  uint32_t bits = 0;  // per lane; reduced only when the wave saw a mismatch

  for (uint64_t i0 = tid - lane; i0 < n4; i0 += stride) {
    const uint64_t i = i0 + lane;
    const uint4 want = cro_pattern_vec4(base_word + (i << 2), seed, invert);
    uint4 got = want;  // lanes past the end compare equal
    if (i < n4) got = s4[i];
    const uint32_t d[4] = {got.x ^ want.x, got.y ^ want.y, got.z ^ want.z,
                           got.w ^ want.w};
    bits |= d[0] | d[1] | d[2] | d[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long mask = __ballot(d[j] != 0);
      if (mask) {
        wave_bad += (unsigned long long)__popcll(mask);
        const unsigned long long first =
            base_word + ((i0 + (uint64_t)(__ffsll(mask) - 1)) << 2) + j;
        wave_first = first < wave_first ? first : wave_first;
      }
    }
  }

  {  // n_words % 4 trailing words, one lane each (first wave of block 0)
    const uint64_t tail0 = n4 << 2;
    uint32_t d = 0;
    if (tid < n_words - tail0)
      d = src[tail0 + tid] ^ cro_pattern_word(base_word + tail0 + tid, seed, invert);
    bits |= d;
    const unsigned long long mask = __ballot(d != 0);
    if (mask) {
      wave_bad += (unsigned long long)__popcll(mask);
      const unsigned long long first =
          base_word + tail0 + (tid - lane) + (uint64_t)(__ffsll(mask) - 1);
      wave_first = first < wave_first ? first : wave_first;
    }
  }

  if (wave_bad) {
    for (int off = 32; off > 0; off >>= 1) bits |= __shfl_xor(bits, off, 64);
    if (lane == 0) {
      atomicAdd(&report->n_bad, wave_bad);
      atomicMin(&report->first_bad, wave_first);
      atomicOr(&report->bits_bad, bits);
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

unsigned grid_for(uint64_t n_words) {
  uint64_t blocks = ((n_words >> 2) + kBlock - 1) / kBlock;
  if (blocks < 1) blocks = 1;  // the tail still needs one workgroup
  if (blocks > kMaxGrid) blocks = kMaxGrid;
  return (unsigned)blocks;
}

void launch_fill(uint32_t* dst, uint64_t n_words, uint64_t base_word, uint32_t seed,
                 uint32_t invert) {
  hipLaunchKernelGGL(pattern_fill_kernel, dim3(grid_for(n_words)), dim3(kBlock), 0, 0,
                     dst, n_words, base_word, seed, invert);
}

void launch_verify(const uint32_t* src, uint64_t n_words, uint64_t base_word,
                   uint32_t seed, uint32_t invert, PatternReport* report) {
  hipLaunchKernelGGL(pattern_verify_kernel, dim3(grid_for(n_words)), dim3(kBlock), 0, 0,
                     src, n_words, base_word, seed, invert, report);
}

const PatternReport kCleanReport = {0, ~0ull, 0, 0};

// Per-device cached context (CtxBase, crohost.h): the pinned link buffer, the
// events and the report word survive between attaches; VRAM does not.
struct IntegCtx : CtxBase {
  PatternReport* d_report = nullptr;
  uint32_t* pinned = nullptr;      // host address
  uint32_t* pinned_dev = nullptr;  // the same memory as the device sees it
  size_t pinned_bytes = 0;
};
IntegCtx g_ictx[kMaxDevices];

// One word of a still-resident device buffer, for the report of a mismatch;
// 0 when the copy fails (the mismatch is what the caller reports either way).
uint32_t device_word(const uint32_t* p) {
  uint32_t got = 0;
  if (hipMemcpy(&got, p, sizeof(got), hipMemcpyDeviceToHost) != hipSuccess) got = 0;
  return got;
}

// Self-test: flips one bit of one word of device memory from the host.
hipError_t flip_device_bit(uint32_t* p, int bit) {
  uint32_t word = 0;
  TRY(hipMemcpy(&word, p, sizeof(word), hipMemcpyDeviceToHost));
  word ^= 1u << bit;
  return hipMemcpy(p, &word, sizeof(word), hipMemcpyHostToDevice);
}

// `got` is the word found at r.first_bad.
int fail_data(CroIntegrityResult* out, Stage which, const PatternReport& r,
              unsigned long long stage_base_word, uint32_t got) {
  const char* stage = kStages[which].name;
  out->ok = 0;
  out->n_bad = r.n_bad;
  out->first_bad_byte = (r.first_bad - stage_base_word) * 4ull;
  out->bits_bad = r.bits_bad;
  out->first_bad_got = got;
  snprintf(out->failed_stage, sizeof(out->failed_stage), "%s", stage);
  snprintf(out->msg, sizeof(out->msg),
           "data mismatch in stage %s: %llu bad words, first at byte %llu, bits 0x%08x",
           stage, out->n_bad, out->first_bad_byte, out->bits_bad);
  return -20;
}

double gbps(double bytes, float ms) { return ms > 0.f ? bytes / (ms * 1e6) : 0.0; }

int run_integrity(int device, const CroIntegrityOpts* opts, CroIntegrityResult* out) {
  CroIntegrityOpts o;
  memset(&o, 0, sizeof(o));
  if (opts) o = *opts;
  const Sizes sizes = normalise_sizes(o.vram_bytes, o.link_bytes, o.chunk_bytes);
  const uint64_t vram_words = sizes.vram_words;
  const uint64_t link_words = sizes.link_words;
  const ChunkPlan plan = chunk_plan(vram_words, sizes.chunk_words);
  const uint32_t seed = o.seed;
  const double floor_gbps = o.link_floor_gbps;
  // Self-test, for tests only: in stage `flip_stage` (-1 = off) the host flips
  // one bit of one word between the stage's write and its compare, so the
  // stage must detect, locate and report through data alone.
  const int flip_stage = o.selftest_stage - 1;
  const int flip_bit = o.selftest_bit;
  const uint64_t flip_word = o.selftest_word;

  std::unique_lock<std::mutex> lock;
  IntegCtx* ctx = enter_device(g_ictx, device, lock, out->msg, sizeof(out->msg));
  if (ctx == nullptr) return -1;
  // after the ordinal, as ever: a bad device is what the message names first
  if (vram_words == 0 || link_words == 0) {
    snprintf(out->msg, sizeof(out->msg), "vram_bytes and link_bytes must be >= 4");
    return -1;
  }
  if (!(floor_gbps >= 0.0)) return bad_arg(out, "link_floor_gbps");  // refuses a NaN too
  if (o.selftest_stage < 0 || o.selftest_stage > kNumStages)
    return bad_arg(out, "selftest_stage");
  if (flip_bit < 0 || flip_bit > 31) return bad_arg(out, "selftest_bit");
  if (o.selftest_pass < 0 || o.selftest_pass > 1 || (o.selftest_pass && flip_stage != kVram))
    return bad_arg(out, "selftest_pass");
  if (flip_stage >= 0 && flip_word >= stage_span_words(flip_stage, sizes))
    return bad_arg(out, "selftest_word");
  // the pinned buffer of a link stage under self-test, after the stage's data
  // is in it and before the compare
  const auto flip_pinned = [&](Stage stage) {
    if (flip_stage == stage) ctx->pinned[flip_word] ^= 1u << flip_bit;
  };
  if (!ctx->ready) {
    CHECK(hipEventCreate(&ctx->e0));
    CHECK(hipEventCreate(&ctx->e1));
    CHECK(hipMalloc(&ctx->d_report, sizeof(PatternReport)));
    ctx->ready = 1;
  }
  if (ctx->pinned_bytes < link_words * 4) {
    if (ctx->pinned) {
      (void)hipHostFree(ctx->pinned);
      ctx->pinned = nullptr;
      ctx->pinned_dev = nullptr;
      ctx->pinned_bytes = 0;
    }
    CHECK(hipHostMalloc(&ctx->pinned, link_words * 4, hipHostMallocMapped));
    CHECK(hipHostGetDevicePointer((void**)&ctx->pinned_dev, ctx->pinned, 0));
    ctx->pinned_bytes = link_words * 4;
    // one untimed round trip with the new buffer: the first copy of a
    // process pays one-time set-up that would understate h2d_dma_gbps
    const size_t warm = link_words * 4 < (1u << 20) ? link_words * 4 : (1u << 20);
    DevBuf<void> tmp;
    CHECK(tmp.alloc(warm));
    CHECK(hipMemcpy(tmp.get(), ctx->pinned, warm, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(ctx->pinned, tmp.get(), warm, hipMemcpyDeviceToHost));
  }
  PatternReport rep;
  float ms = 0.f;
  // VRAM held by this run; released on every way out
  std::vector<DevBuf<uint32_t>> chunks;
  DevBuf<uint32_t> dlink;

  // -- VRAM ------------------------------------------------------------------
  double t0 = now_ms();
  for (uint64_t c = 0; c < plan.count(); ++c) {
    chunks.emplace_back();
    CHECK(chunks.back().alloc((plan.words(c) * 4 + 15) & ~15ull));
  }
  out->vram_chunks = (int)chunks.size();
  // word `w` of the span, in the chunk that holds it
  const auto vram_word = [&](uint64_t w) {
    const ChunkPos pos = locate(plan, w);
    return chunks[pos.chunk].get() + pos.word;
  };
  float fill_ms = 0.f, verify_ms = 0.f;
  for (uint32_t pass = 0; pass < 2; ++pass) {
    const StagePattern pat = stage_pattern(kVram, pass, seed);
    // every chunk in one timed window, at its place in the span's word count
    const auto fill_all = [&] {
      for (size_t c = 0; c < chunks.size(); ++c)
        launch_fill(chunks[c].get(), plan.words(c), plan.base(c), pat.seed, pat.invert);
    };
    const auto verify_all = [&] {
      for (size_t c = 0; c < chunks.size(); ++c)
        launch_verify(chunks[c].get(), plan.words(c), plan.base(c), pat.seed, pat.invert,
                      ctx->d_report);
    };
    CHECK(timed_ms(*ctx, &ms, fill_all));  // synchronised when it returns
    fill_ms += ms;
    if (flip_stage == kVram && (uint32_t)o.selftest_pass == pass)
      CHECK(flip_device_bit(vram_word(flip_word), flip_bit));

    CHECK(hipMemcpy(ctx->d_report, &kCleanReport, sizeof(rep), hipMemcpyHostToDevice));
    CHECK(timed_ms(*ctx, &ms, verify_all));
    verify_ms += ms;
    CHECK(hipMemcpy(&rep, ctx->d_report, sizeof(rep), hipMemcpyDeviceToHost));
    out->vram_passes = (int)pass + 1;
    out->vram_bytes_verified += (long long)(vram_words * 4);
    out->vram_n_bad += rep.n_bad;
    if (rep.n_bad)
      return fail_data(out, kVram, rep, 0,
                       rep.first_bad < vram_words ? device_word(vram_word(rep.first_bad)) : 0u);
  }
  out->vram_fill_gbps = gbps(2.0 * vram_words * 4, fill_ms);
  out->vram_verify_gbps = gbps(2.0 * vram_words * 4, verify_ms);
  for (DevBuf<uint32_t>& chunk : chunks) CHECK(chunk.free());
  chunks.clear();
  out->t_vram_ms = now_ms() - t0;

  // -- link, copy engines ------------------------------------------------------
  // (a copy that fails inside a timed window is what timed_ms reports)
  t0 = now_ms();
  const double lbytes = (double)(link_words * 4);
  CHECK(dlink.alloc((link_words * 4 + 15) & ~15ull));
  StagePattern pat = stage_pattern(kH2dDma, 0, seed);
  host_fill(ctx->pinned, link_words, pat.seed, pat.invert);
  const auto h2d_copy = [&] {
    (void)hipMemcpy(dlink.get(), ctx->pinned, link_words * 4, hipMemcpyHostToDevice);
  };
  CHECK(timed_ms(*ctx, &ms, h2d_copy));
  out->h2d_dma_gbps = gbps(lbytes, ms);
  if (flip_stage == kH2dDma) CHECK(flip_device_bit(dlink.get() + flip_word, flip_bit));
  CHECK(hipMemcpy(ctx->d_report, &kCleanReport, sizeof(rep), hipMemcpyHostToDevice));
  launch_verify(dlink.get(), link_words, 0, pat.seed, pat.invert, ctx->d_report);
  CHECK(hipGetLastError());
  CHECK(hipMemcpy(&rep, ctx->d_report, sizeof(rep), hipMemcpyDeviceToHost));
  out->link_passes = 1;
  out->h2d_dma_bytes_verified = (long long)(link_words * 4);
  out->h2d_dma_n_bad = rep.n_bad;
  if (rep.n_bad)
    return fail_data(out, kH2dDma, rep, 0,
                     rep.first_bad < link_words ? device_word(dlink.get() + rep.first_bad) : 0u);

  pat = stage_pattern(kD2hDma, 0, seed);
  launch_fill(dlink.get(), link_words, 0, pat.seed, pat.invert);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  const auto d2h_copy = [&] {
    (void)hipMemcpy(ctx->pinned, dlink.get(), link_words * 4, hipMemcpyDeviceToHost);
  };
  CHECK(timed_ms(*ctx, &ms, d2h_copy));
  out->d2h_dma_gbps = gbps(lbytes, ms);
  flip_pinned(kD2hDma);
  rep = host_verify(ctx->pinned, link_words, pat.seed, pat.invert);
  out->d2h_dma_bytes_verified = (long long)(link_words * 4);
  out->d2h_dma_n_bad = rep.n_bad;
  if (rep.n_bad) return fail_data(out, kD2hDma, rep, 0, ctx->pinned[rep.first_bad]);
  CHECK(dlink.free());
  out->t_link_dma_ms = now_ms() - t0;

  // -- link, shader loads and stores (complement pattern) ----------------------
  t0 = now_ms();
  pat = stage_pattern(kH2dKernel, 0, seed);
  host_fill(ctx->pinned, link_words, pat.seed, pat.invert);
  flip_pinned(kH2dKernel);
  CHECK(hipMemcpy(ctx->d_report, &kCleanReport, sizeof(rep), hipMemcpyHostToDevice));
  const auto h2d_verify = [&] {
    launch_verify(ctx->pinned_dev, link_words, 0, pat.seed, pat.invert, ctx->d_report);
  };
  CHECK(timed_ms(*ctx, &ms, h2d_verify));
  out->h2d_kernel_gbps = gbps(lbytes, ms);
  CHECK(hipMemcpy(&rep, ctx->d_report, sizeof(rep), hipMemcpyDeviceToHost));
  out->h2d_kernel_bytes_verified = (long long)(link_words * 4);
  out->h2d_kernel_n_bad = rep.n_bad;
  if (rep.n_bad)
    return fail_data(out, kH2dKernel, rep, 0,
                     rep.first_bad < link_words ? ctx->pinned[rep.first_bad] : 0u);

  pat = stage_pattern(kD2hKernel, 0, seed);
  const auto d2h_fill = [&] {
    launch_fill(ctx->pinned_dev, link_words, 0, pat.seed, pat.invert);
  };
  CHECK(timed_ms(*ctx, &ms, d2h_fill));
  out->d2h_kernel_gbps = gbps(lbytes, ms);
  CHECK(hipDeviceSynchronize());
  flip_pinned(kD2hKernel);
  rep = host_verify(ctx->pinned, link_words, pat.seed, pat.invert);
  out->d2h_kernel_bytes_verified = (long long)(link_words * 4);
  out->d2h_kernel_n_bad = rep.n_bad;
  if (rep.n_bad) return fail_data(out, kD2hKernel, rep, 0, ctx->pinned[rep.first_bad]);
  out->t_link_kernel_ms = now_ms() - t0;

  if (floor_gbps > 0.0) {
    const struct { const char* stage; double rate; } rates[] = {
        {"h2d_dma", out->h2d_dma_gbps},       {"d2h_dma", out->d2h_dma_gbps},
        {"h2d_kernel", out->h2d_kernel_gbps}, {"d2h_kernel", out->d2h_kernel_gbps}};
    for (const auto& r : rates) {
      if (r.rate < floor_gbps) {
        snprintf(out->failed_stage, sizeof(out->failed_stage), "%s", r.stage);
        snprintf(out->msg, sizeof(out->msg),
                 "link rate %.1f GB/s in stage %s below floor %.1f GB/s", r.rate, r.stage,
                 floor_gbps);
        return -21;
      }
    }
  }
  out->ok = 1;
  snprintf(out->msg, sizeof(out->msg), "ok");
  return 0;
}

// Raw entries: the buffer is rounded up to whole vectors and followed by a
// guard band, all preset to 0xA5 bytes, so a store or a load past n_words
// shows in data (tests/test_probe_integrity.py: 0xA5A5A5A5 is the pattern at
// none of those indices).
constexpr size_t kGuardBytes = 64 * 16;
constexpr unsigned char kGuardByte = 0xA5;

size_t raw_alloc_bytes(unsigned long long n_words) {
  return (size_t)((n_words * 4 + 15) & ~15ull) + kGuardBytes;
}

}  // namespace

extern "C" int cro_probe_integrity(int device, const struct CroIntegrityOpts* opts,
                                   struct CroIntegrityResult* out) {
  memset(out, 0, sizeof(*out));
  out->first_bad_byte = ~0ull;
  const double t0 = now_ms();
  out->rc = run_integrity(device, opts, out);
  out->t_total_ms = now_ms() - t0;
  return out->rc;
}

extern "C" int cro_probe_pattern_fill(int device, unsigned int seed, int invert,
                                      unsigned long long base_word,
                                      unsigned long long n_words, unsigned int* host_out,
                                      int* guard_ok) {
  if (n_words == 0 || host_out == nullptr || guard_ok == nullptr) return -10;
  *guard_ok = 0;
  if (hipSetDevice(device) != hipSuccess) return -1;
  const size_t bytes = raw_alloc_bytes(n_words);
  const size_t after = bytes - (size_t)n_words * 4;  // slack words and guard band
  DevBuf<uint32_t> d;
  std::vector<unsigned char> back(after);
  const auto run = [&]() -> hipError_t {
    TRY(d.alloc(bytes));
    TRY(hipMemset(d.get(), kGuardByte, bytes));
    launch_fill(d.get(), n_words, base_word, seed, invert ? 1u : 0u);
    TRY(hipGetLastError());
    TRY(hipMemcpy(host_out, d.get(), n_words * 4, hipMemcpyDeviceToHost));
    return hipMemcpy(back.data(), d.get() + n_words, after, hipMemcpyDeviceToHost);
  };
  if (run() != hipSuccess) return -1;
  int ok = 1;
  for (size_t i = 0; i < after; ++i) ok &= back[i] == kGuardByte;
  *guard_ok = ok;
  return 0;
}

extern "C" int cro_probe_pattern_verify(int device, unsigned int seed, int invert,
                                        unsigned long long base_word,
                                        unsigned long long n_words,
                                        const unsigned int* host_in,
                                        unsigned long long* n_bad,
                                        unsigned long long* first_bad,
                                        unsigned int* bits_bad) {
  if (n_words == 0 || host_in == nullptr) return -10;
  if (hipSetDevice(device) != hipSuccess) return -1;
  DevBuf<uint32_t> d;
  DevBuf<PatternReport> d_rep;
  PatternReport rep = kCleanReport;
  const auto run = [&]() -> hipError_t {
    TRY(d.alloc(raw_alloc_bytes(n_words)));
    TRY(d_rep.alloc(sizeof(rep)));
    TRY(hipMemset(d.get(), kGuardByte, raw_alloc_bytes(n_words)));
    TRY(hipMemcpy(d.get(), host_in, n_words * 4, hipMemcpyHostToDevice));
    TRY(hipMemcpy(d_rep.get(), &rep, sizeof(rep), hipMemcpyHostToDevice));
    launch_verify(d.get(), n_words, base_word, seed, invert ? 1u : 0u, d_rep.get());
    TRY(hipGetLastError());
    return hipMemcpy(&rep, d_rep.get(), sizeof(rep), hipMemcpyDeviceToHost);
  };
  if (run() != hipSuccess) return -1;
  if (n_bad) *n_bad = rep.n_bad;
  if (first_bad) *first_bad = rep.first_bad;
  if (bits_bad) *bits_bad = rep.bits_bad;
  return 0;
}
