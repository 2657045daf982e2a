// cro_amd gfx950 scrub stage: overwrite and verify a device's VRAM before it
// is drained (croscrub.h says what that covers and what it does not).
//
//   acquire — all the VRAM the driver hands over, by the plan of
//             croscrubplan.h; every chunk stays resident to the end, so the
//             run cannot get the same pages twice and the early chunks have
//             left the last-level cache before they are verified.
//   census  — count the words that differ from the fill word as handed over
//             (tells a site whether its driver already wipes; never gated).
//   fill    — store the fill word everywhere, one event-timed window.
//   verify  — load every word back, one event-timed window.
//
// Two kernels without pattern arithmetic: a store-only fill and a load-only
// verify whose common path is one OR and one ballot per 16-byte vector.
//
// A library of its own, libcroscrub.so (cro_amd/hip/build.py: build_scrub);
// host plumbing shared with libcroprobe.so's stages in crohost.h.

#include <hip/hip_runtime.h>
#include <cstring>
#include <utility>
#include <vector>

#include "crohost.h"
#include "crointegrity.h"
#include "croscrub.h"
#include "croscrubplan.h"

namespace {

using crointegrity::PatternReport;
using namespace croscrub;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// A workgroup of 256 lanes covers kUnroll x 256 vectors per trip (4096 words,
// 16 KiB); 1024 workgroups (4 on each of the 256 CUs) cover 16 MiB per grid
// pass, grid-stride for the rest.
constexpr int kUnroll = 4;
constexpr uint64_t kSpanVecs = (uint64_t)kUnroll * kBlock;
constexpr unsigned kMaxGrid = 1024;

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void scrub_fill_kernel(uint32_t* __restrict__ dst,
                                                            uint64_t n_words, uint32_t word) {
  const uint64_t n4 = n_words >> 2;
  u32x4* __restrict__ d4 = reinterpret_cast<u32x4*>(dst);
  const u32x4 v = {word, word, word, word};
  const uint64_t stride = (uint64_t)gridDim.x * kSpanVecs;
  for (uint64_t s0 = (uint64_t)blockIdx.x * kSpanVecs; s0 < n4; s0 += stride) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint64_t i = s0 + (uint64_t)u * kBlock + threadIdx.x;
      if (i < n4) __builtin_nontemporal_store(v, &d4[i]);
    }
  }
  const uint64_t tail0 = n4 << 2;  // n_words % 4 trailing words, one lane each
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid < n_words - tail0) dst[tail0 + tid] = word;
}

// The loop runs on the workgroup's span index, which every lane shares, so
// all 64 lanes of a wave reach every ballot.  Per unrolled slot the wave
// ballots one OR of the vector's four differences; only when that is
// non-zero do the four per-word ballots run, which give the count
// (__popcll — a 32-bit popcount would drop lanes 32-63), the first bad word
// and the bad bits.  A wave that saw nothing bad issues no atomic at all; one
// that did issues one add, one min and one or.
__global__ __launch_bounds__(kBlock) void scrub_verify_kernel(
    const uint32_t* __restrict__ src, uint64_t n_words, uint64_t base_word, uint32_t word,
    PatternReport* __restrict__ report) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave_vec0 = threadIdx.x - lane;  // of the wave's lane 0, within a slot
  const uint64_t n4 = n_words >> 2;
  const u32x4* __restrict__ s4 = reinterpret_cast<const u32x4*>(src);
  const u32x4 want = {word, word, word, word};
  const uint64_t stride = (uint64_t)gridDim.x * kSpanVecs;

  unsigned long long wave_bad = 0;
  unsigned long long wave_first = ~0ull;
  uint32_t bits = 0;  // per lane; reduced only when the wave saw a mismatch

  for (uint64_t s0 = (uint64_t)blockIdx.x * kSpanVecs; s0 < n4; s0 += stride) {
    u32x4 d[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint64_t i = s0 + (uint64_t)u * kBlock + threadIdx.x;
      u32x4 got = want;  // lanes past the end compare equal
      if (i < n4) got = __builtin_nontemporal_load(&s4[i]);
      d[u] = got ^ want;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint32_t any = d[u].x | d[u].y | d[u].z | d[u].w;
      if (__ballot(any != 0) == 0) continue;  // wave-uniform
      bits |= any;
      const uint64_t vec0 = s0 + (uint64_t)u * kBlock + wave_vec0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned long long mask = __ballot(d[u][j] != 0);
        if (mask) {
          wave_bad += (unsigned long long)__popcll(mask);
          const unsigned long long first =
              base_word + ((vec0 + (uint64_t)(__ffsll(mask) - 1)) << 2) + j;
          wave_first = first < wave_first ? first : wave_first;
        }
      }
    }
  }

  {  // n_words % 4 trailing words, one lane each (first wave of block 0)
    const uint64_t tail0 = n4 << 2;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t dt = 0;
    if (tid < n_words - tail0) dt = src[tail0 + tid] ^ word;
    const unsigned long long mask = __ballot(dt != 0);
    if (mask) {
      bits |= dt;
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

// grid_blocks 0: one workgroup per span of the buffer, at most kMaxGrid
unsigned grid_for(uint64_t n_words, int grid_blocks) {
  if (grid_blocks > 0) return (unsigned)grid_blocks;
  uint64_t blocks = ((n_words >> 2) + kSpanVecs - 1) / kSpanVecs;
  if (blocks < 1) blocks = 1;  // the tail still needs one workgroup
  if (blocks > kMaxGrid) blocks = kMaxGrid;
  return (unsigned)blocks;
}

void launch_fill(uint32_t* dst, uint64_t n_words, uint32_t word, int grid_blocks) {
  hipLaunchKernelGGL(scrub_fill_kernel, dim3(grid_for(n_words, grid_blocks)), dim3(kBlock), 0,
                     0, dst, n_words, word);
}

void launch_verify(const uint32_t* src, uint64_t n_words, uint64_t base_word, uint32_t word,
                   int grid_blocks, PatternReport* report) {
  hipLaunchKernelGGL(scrub_verify_kernel, dim3(grid_for(n_words, grid_blocks)), dim3(kBlock),
                     0, 0, src, n_words, base_word, word, report);
}

const PatternReport kCleanReport = {0, ~0ull, 0, 0};

// Per-device cached context (CtxBase, crohost.h): the events and the report
// survive between runs; VRAM does not.
struct ScrubCtx : CtxBase {
  PatternReport* d_report = nullptr;
};
ScrubCtx g_sctx[kMaxDevices];

// One word of a still-resident device buffer, for the report of residue;
// 0 when the copy fails (the residue is what the caller reports either way).
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

double gbps(double bytes, float ms) { return ms > 0.f ? bytes / (ms * 1e6) : 0.0; }

constexpr unsigned char kPresetByte = 0xA5;  // self-test modes 2 and 3; the raw entries' guards

int run_scrub(int device, const CroScrubOpts* opts, CroScrubResult* out) {
  CroScrubOpts o;
  memset(&o, 0, sizeof(o));
  if (opts) o = *opts;
  const uint32_t fill_word = o.fill_word;

  std::unique_lock<std::mutex> lock;
  ScrubCtx* ctx = enter_device(g_sctx, device, lock, out->msg, sizeof(out->msg));
  if (ctx == nullptr) return -1;
  if (!(o.min_fraction >= 0.0 && o.min_fraction <= 1.0))  // refuses a NaN too
    return bad_arg(out, "min_fraction");
  if (o.selftest_mode < 0 || o.selftest_mode > 3) return bad_arg(out, "selftest_mode");
  if (o.selftest_bit < 0 || o.selftest_bit > 31) return bad_arg(out, "selftest_bit");
  if (o.selftest_refuse_at < 0) return bad_arg(out, "selftest_refuse_at");
  if (!ctx->ready) {
    CHECK(hipEventCreate(&ctx->e0));
    CHECK(hipEventCreate(&ctx->e1));
    CHECK(hipMalloc(&ctx->d_report, sizeof(PatternReport)));
    ctx->ready = 1;
  }

  // -- acquire -----------------------------------------------------------------
  size_t free_bytes = 0, total_bytes = 0;
  CHECK(hipMemGetInfo(&free_bytes, &total_bytes));
  out->vram_total = (long long)total_bytes;
  out->vram_free_before = (long long)free_bytes;
  const uint64_t target = target_bytes(free_bytes, o.reserve_bytes, o.max_bytes);
  out->bytes_target = (long long)target;
  if (target == 0) {
    snprintf(out->msg, sizeof(out->msg),
             "nothing to scrub: %zu bytes free, %llu reserved for the runtime", free_bytes,
             (unsigned long long)normalise_reserve(o.reserve_bytes));
    return -1;
  }
  if (o.selftest_mode == 1 && o.selftest_word >= target / 4) return bad_arg(out, "selftest_word");

  // VRAM held by this run; released on every way out
  std::vector<DevBuf<uint32_t>> chunks;
  ChunkList list;
  double t0 = now_ms();
  int request_no = 0;
  const PlanStats plan = acquire(target, normalise_chunk(o.chunk_bytes), [&](uint64_t bytes) {
    if (++request_no == o.selftest_refuse_at) return false;
    DevBuf<uint32_t> buf;
    if (buf.alloc(bytes) != hipSuccess) {
      (void)hipGetLastError();  // a refusal is not a failure
      return false;
    }
    chunks.push_back(std::move(buf));
    list.add(bytes / 4);
    return true;
  });
  out->t_alloc_ms = now_ms() - t0;
  out->chunks = (int)plan.chunks;
  out->alloc_refusals = (int)plan.refusals;
  const uint64_t span_words = list.span_words();
  const double span_bytes = (double)span_words * 4.0;
  if (span_words == 0) {
    snprintf(out->msg, sizeof(out->msg), "nothing to scrub: the driver granted no allocation");
    return -1;
  }
  if (o.selftest_mode == 1 && o.selftest_word >= span_words)
    return bad_arg(out, "selftest_word");
  // word `w` of the span, in the chunk that holds it
  const auto span_word = [&](uint64_t w) {
    const ChunkList::Pos pos = list.locate(w);
    return chunks[pos.chunk].get() + pos.word;
  };
  if (o.selftest_mode >= 2)
    for (size_t c = 0; c < chunks.size(); ++c)
      CHECK(hipMemset(chunks[c].get(), kPresetByte, list.words(c) * 4));

  // every chunk in one timed window, at its place in the span's word count
  const auto verify_all = [&] {
    for (size_t c = 0; c < chunks.size(); ++c)
      launch_verify(chunks[c].get(), list.words(c), list.base(c), fill_word, 0, ctx->d_report);
  };
  const auto fill_all = [&] {
    for (size_t c = 0; c < chunks.size(); ++c)
      launch_fill(chunks[c].get(), list.words(c), fill_word, 0);
  };
  PatternReport rep;
  float ms = 0.f;

  // -- census ------------------------------------------------------------------
  CHECK(hipMemcpy(ctx->d_report, &kCleanReport, sizeof(rep), hipMemcpyHostToDevice));
  CHECK(timed_ms(*ctx, &ms, verify_all));  // synchronised when it returns
  CHECK(hipMemcpy(&rep, ctx->d_report, sizeof(rep), hipMemcpyDeviceToHost));
  out->dirty_words_before = rep.n_bad;
  out->census_gbps = gbps(span_bytes, ms);

  // -- fill --------------------------------------------------------------------
  if (o.selftest_mode != 2) {
    CHECK(timed_ms(*ctx, &ms, fill_all));
    out->bytes_scrubbed = (long long)(span_words * 4);
    out->fill_gbps = gbps(span_bytes, ms);
  }
  if (o.selftest_mode == 1) CHECK(flip_device_bit(span_word(o.selftest_word), o.selftest_bit));

  // -- verify ------------------------------------------------------------------
  CHECK(hipMemcpy(ctx->d_report, &kCleanReport, sizeof(rep), hipMemcpyHostToDevice));
  CHECK(timed_ms(*ctx, &ms, verify_all));
  CHECK(hipMemcpy(&rep, ctx->d_report, sizeof(rep), hipMemcpyDeviceToHost));
  out->bytes_verified = (long long)(span_words * 4);
  out->verify_gbps = gbps(span_bytes, ms);
  out->n_bad = rep.n_bad;
  out->bits_bad = rep.bits_bad;
  if (rep.n_bad) {
    out->first_bad_byte = rep.first_bad * 4ull;
    out->first_bad_got = rep.first_bad < span_words ? device_word(span_word(rep.first_bad)) : 0u;
  }
  out->fraction = total_bytes ? (double)out->bytes_scrubbed / (double)total_bytes : 0.0;

  for (DevBuf<uint32_t>& chunk : chunks) CHECK(chunk.free());
  chunks.clear();

  // -- gates -------------------------------------------------------------------
  if (out->n_bad) {
    snprintf(out->msg, sizeof(out->msg),
             "residue after scrub: %llu bad words, first at byte %llu (found 0x%08x), "
             "bits 0x%08x",
             out->n_bad, out->first_bad_byte, out->first_bad_got, out->bits_bad);
    return -40;
  }
  if (o.min_fraction > 0.0 && out->fraction < o.min_fraction) {
    snprintf(out->msg, sizeof(out->msg), "scrubbed fraction %.4f of VRAM below floor %.4f",
             out->fraction, o.min_fraction);
    return -41;
  }
  out->ok = 1;
  snprintf(out->msg, sizeof(out->msg), "ok");
  return 0;
}

// Raw entries: the buffer is rounded up to whole vectors and lies between two
// guard bands, all preset to 0xA5 bytes, so a store or a load outside the
// n_words shows in data.
constexpr size_t kGuardBytes = 64 * 16;

size_t raw_data_bytes(unsigned long long n_words) {
  return (size_t)((n_words * 4 + 15) & ~15ull);
}

bool raw_args_ok(unsigned long long n_words, int grid_blocks) {
  return n_words != 0 && n_words <= (1ull << 32) && grid_blocks >= 0 &&
         grid_blocks <= (int)kMaxGrid;
}

}  // namespace

extern "C" int cro_scrub_run(int device, const struct CroScrubOpts* opts,
                             struct CroScrubResult* out) {
  memset(out, 0, sizeof(*out));
  out->first_bad_byte = ~0ull;
  const double t0 = now_ms();
  out->rc = run_scrub(device, opts, out);
  out->t_total_ms = now_ms() - t0;
  return out->rc;
}

extern "C" int cro_scrub_fill(int device, unsigned long long n_words, unsigned int fill_word,
                              int grid_blocks, unsigned int* host_out, int* guard_ok) {
  if (!raw_args_ok(n_words, grid_blocks) || host_out == nullptr || guard_ok == nullptr)
    return -10;
  *guard_ok = 0;
  if (hipSetDevice(device) != hipSuccess) return -1;
  const size_t data = raw_data_bytes(n_words);
  const size_t bytes = kGuardBytes + data + kGuardBytes;
  const size_t after = data - (size_t)n_words * 4 + kGuardBytes;  // slack words and guard band
  DevBuf<unsigned char> d;
  std::vector<unsigned char> guards(kGuardBytes + after);
  const auto run = [&]() -> hipError_t {
    TRY(d.alloc(bytes));
    TRY(hipMemset(d.get(), kPresetByte, bytes));
    uint32_t* words = reinterpret_cast<uint32_t*>(d.get() + kGuardBytes);
    launch_fill(words, n_words, fill_word, grid_blocks);
    TRY(hipGetLastError());
    TRY(hipMemcpy(host_out, words, n_words * 4, hipMemcpyDeviceToHost));
    TRY(hipMemcpy(guards.data(), d.get(), kGuardBytes, hipMemcpyDeviceToHost));
    return hipMemcpy(guards.data() + kGuardBytes, words + n_words, after,
                     hipMemcpyDeviceToHost);
  };
  if (run() != hipSuccess) return -1;
  int ok = 1;
  for (unsigned char b : guards) ok &= b == kPresetByte;
  *guard_ok = ok;
  return 0;
}

extern "C" int cro_scrub_verify(int device, const unsigned int* host_in,
                                unsigned long long n_words, unsigned long long base_word,
                                unsigned int fill_word, int grid_blocks,
                                unsigned long long* n_bad, unsigned long long* first_bad,
                                unsigned int* bits_bad) {
  if (!raw_args_ok(n_words, grid_blocks) || host_in == nullptr) return -10;
  if (hipSetDevice(device) != hipSuccess) return -1;
  const size_t bytes = kGuardBytes + raw_data_bytes(n_words) + kGuardBytes;
  DevBuf<unsigned char> d;
  DevBuf<PatternReport> d_rep;
  PatternReport rep = kCleanReport;
  const auto run = [&]() -> hipError_t {
    TRY(d.alloc(bytes));
    TRY(d_rep.alloc(sizeof(rep)));
    TRY(hipMemset(d.get(), kPresetByte, bytes));
    uint32_t* words = reinterpret_cast<uint32_t*>(d.get() + kGuardBytes);
    TRY(hipMemcpy(words, host_in, n_words * 4, hipMemcpyHostToDevice));
    TRY(hipMemcpy(d_rep.get(), &rep, sizeof(rep), hipMemcpyHostToDevice));
    launch_verify(words, n_words, base_word, fill_word, grid_blocks, d_rep.get());
    TRY(hipGetLastError());
    return hipMemcpy(&rep, d_rep.get(), sizeof(rep), hipMemcpyDeviceToHost);
  };
  if (run() != hipSuccess) return -1;
  if (n_bad) *n_bad = rep.n_bad;
  if (first_bad) *first_bad = rep.first_bad;
  if (bits_bad) *bits_bad = rep.bits_bad;
  return 0;
}

extern "C" unsigned long long cro_scrub_grid_pass_words(void) {
  return (unsigned long long)kMaxGrid * kSpanVecs * 4ull;
}
