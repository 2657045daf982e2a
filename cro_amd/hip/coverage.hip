// cro_amd gfx950 compute-coverage probe: exact checks on every CU and SIMD,
// with fault location.
//
// The quick probe (probe.hip) compares one wave's f32 MFMA on one CU; its
// bf16 rate kernel runs everywhere and compares nothing; no probe kernel
// touches LDS.  This stage launches one 256-thread workgroup per CU — the
// default dynamic-LDS request is a CU's whole 160 KiB, which is what places
// one workgroup per CU and, with four waves, one wave per SIMD — and each
// wave, `iters` times:
//
//   mfma_f32   v_mfma_f32_16x16x4_f32, K = 64, against the host fmaf chain
//   mfma_i8    v_mfma_i32_16x16x64_i8, K = 256, against an integer product
//   mfma_bf16  v_mfma_f32_32x32x16_bf16, K = 64, small integers, so the f32
//              result is exact in any summation order
//   lds        the workgroup writes the cropattern.h word of every LDS word
//              with 16-byte stores, verifies with 16-byte loads, then the
//              complement
//
// Every comparison is exact and made on the device, each lane on its own
// registers; mismatches are counted per wave with a 64-lane ballot and a
// 64-bit popcount (as integrity.hip).  Each wave reads where it ran
// (XCC_ID, HW_ID) and lane 0 writes one CroCoverageRecord.  Workgroups are
// independent: no inter-workgroup communication, no spin, no grid barrier.
// The host aggregates the records (crocoverage.h) and launches the same grid
// again, a bounded number of times, while some CU or SIMD is still unseen.
// The location is for the report only; HIP promises nothing about placement,
// so coverage gates only when the caller sets min_cu_fraction.
//
// For tests the kernel is a template: its second instantiation can make LDS
// words wrong between fill and verify (self-test modes 3 and 4) or copy LDS
// out after a fill (cro_probe_compute_lds_dump), and the host can hand the
// kernel the caller's expected tiles (cro_probe_compute_tiles); croprobe.h.
// A run without a plant launches the first instantiation.
//
// Compiled with probe.hip and integrity.hip into libcroprobe.so; host plumbing
// shared with them in crohost.h, one wave's matrix products and result maps
// shared with probe.hip in cromfma.h.

#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>

#include "crohost.h"
#include "cromfma.h"
#include "cropattern.h"
#include "croprobe.h"

namespace {

constexpr int kWaves = kBlock / 64;
// ≈0.035 ms per repeat on an MI355X: 16 keeps the stage at the cost of one of
// the quick probe's rate sections (profiles/compute_probe_mi355x.md)
constexpr int kDefaultIters = 16;
constexpr int kDefaultRounds = 4;
constexpr int kMaxRounds = 64;
constexpr int kMaxGrid = 1 << 16;
constexpr int kMaxIters = 1 << 16;
// the dump entry's guard: 256 words after the marched ones (as croldsscrub.h)
constexpr uint32_t kGuardWord = 0xA5A5A5A5u;
constexpr int kGuardBytes = 1024;
constexpr int kMaxDumpGrid = 8;

// one wave of the coverage kernel's i8 or bf16 product (cromfma.h), stored
// through the result maps: the raw tile entry's kernel
__global__ __launch_bounds__(64) void mfma_tile_kernel(int kind, const void* A, const void* B,
                                                       void* D, int K) {
  const uint32_t lane = threadIdx.x;  // exactly one wave of 64
  if (kind == 1) {
    const i32x4 acc = wave_mfma_i8((const int8_t*)A, (const int8_t*)B, K, lane);
    for (int r = 0; r < 4; ++r) ((int*)D)[mfma_elem16(lane, r)] = acc[r];
  } else {
    const f32x16 acc = wave_mfma_bf16((const uint16_t*)A, (const uint16_t*)B, K, lane);
    for (int r = 0; r < 16; ++r) ((float*)D)[mfma_elem32(lane, r)] = acc[r];
  }
}

// ---------------------------------------------------------------------------
// coverage kernel
// ---------------------------------------------------------------------------

struct CovParams {
  const float* A32;
  const float* B32;
  const float* E32;  // expected 16x16
  const int8_t* A8;
  const int8_t* B8;
  const int* E8;  // expected 16x16
  const uint16_t* A16;
  const uint16_t* B16;
  const float* E16;  // expected 32x32
  CroCoverageRecord* records;  // this round's grid_blocks * 4 records
  uint32_t lds_words;
  uint32_t iters;
  uint32_t seed;
  uint32_t inj_mode;  // self-test, see croprobe.h
  uint32_t inj_test;
  uint32_t inj_elem;
  uint32_t inj_flip;  // 1 << selftest_bit
  uint32_t inj_key;
  // test seams, read by coverage_kernel<true> only
  uint32_t inj_span;   // modes 3 and 4: words planted from inj_elem on
  uint32_t inj_pass;   // 0 pattern, 1 complement, 2 both
  uint32_t* dump_out;  // not null: copy LDS out after the fill of dump_pass, and return
  uint32_t dump_pass;
  uint32_t guard_vecs;  // vectors after the marched ones, preset and counted
  unsigned int* guard_bad;
};

// What one wave found in one test.  n_bad is wave-uniform (ballot counts);
// first and bits are per lane until reduce().
struct Tally {
  uint32_t n_bad = 0;
  uint32_t first = ~0u;
  uint32_t bits = 0;

  __device__ void add(uint32_t diff, uint32_t elem) {
    bits |= diff;
    const unsigned long long mask = __ballot(diff != 0);
    if (mask) {
      n_bad += (uint32_t)__popcll(mask);
      if (diff) first = elem < first ? elem : first;
    }
  }
  // every lane of the wave calls it (n_bad is uniform, so the branch is)
  __device__ void reduce() {
    if (!n_bad) return;
    for (int off = 32; off > 0; off >>= 1) {
      bits |= __shfl_xor(bits, off, 64);
      const uint32_t other = __shfl_xor(first, off, 64);
      first = other < first ? other : first;
    }
  }
};

__device__ inline uint32_t f32_bits(float x) { return __builtin_bit_cast(uint32_t, x); }

// Expected content of LDS vector v.  A function of the 32-bit vector index on
// purpose: with the widening written at the two call sites the compiler folds
// the march's address arithmetic differently, and the kernel measured about
// 1 % slower on an MI355X.
__device__ inline uint4 lds_want(uint64_t base_word, uint32_t v, uint32_t seed,
                                 uint32_t invert) {
  return cro_pattern_vec4(base_word + ((uint64_t)v << 2), seed, invert);
}

// kSeams = false is the stage's kernel.  kSeams = true adds, between the
// fill's barrier and the verify loop, what the tests of the march need: the
// LDS plant of self-test modes 3 and 4 and the dump (croprobe.h).  The fill
// and verify loops are the same source in both.
template <bool kSeams>
__global__ __launch_bounds__(kBlock) void coverage_kernel(CovParams p) {
  // all LDS is dynamic, so its base stays 16-byte aligned for the b128 accesses
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* lds4 = reinterpret_cast<uint4*>(smem);

  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t xcc_id, hw_id;  // for the report only
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
  // self-test mode 2 flips computed values on the waves of one CU; mode 1 is
  // done on the host except for LDS, whose expected words are computed here
  const bool inj_computed = p.inj_mode == 2 && cro_cov_cu_key(xcc_id, hw_id) == p.inj_key;
  const bool inj_lds =
      p.inj_test == CRO_COV_TEST_LDS && (p.inj_mode == 1 || inj_computed);
  const uint32_t inj_vec = p.inj_elem >> 2, inj_word = p.inj_elem & 3;

  // the elements this lane holds
  uint32_t elem16[4], elem32[16];
  float want_f32[4], want_bf16[16];
  int want_i8[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    elem16[r] = mfma_elem16(lane, r);
    want_f32[r] = p.E32[elem16[r]];
    want_i8[r] = p.E8[elem16[r]];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    elem32[r] = mfma_elem32(lane, r);
    want_bf16[r] = p.E16[elem32[r]];
  }

  Tally t_f32, t_i8, t_bf16, t_lds;
  const uint32_t n4 = p.lds_words >> 2;
  const uint64_t lds_base = (uint64_t)blockIdx.x * p.lds_words;

  // A workgroup runs on one CU, so this is the same in all of its threads:
  // the plant's barrier below is reached by every one of them or by none.
  bool plant = false;
  if constexpr (kSeams) {
    plant = p.inj_mode == 3 || (p.inj_mode == 4 && cro_cov_cu_key(xcc_id, hw_id) == p.inj_key);
    for (uint32_t v = n4 + tid; v < n4 + p.guard_vecs; v += kBlock)
      lds4[v] = make_uint4(kGuardWord, kGuardWord, kGuardWord, kGuardWord);
  }

  for (uint32_t it = 0; it < p.iters; ++it) {
    // an offset of zero the compiler cannot see through: the products are
    // recomputed, operands reloaded, in every iteration
    uint32_t z = 0;
    asm volatile("" : "+v"(z));

    {
      const f32x4 acc = wave_mfma_f32(p.A32 + z, p.B32 + z, CRO_COV_F32_K, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        uint32_t got = f32_bits(acc[r]);
        if (inj_computed && p.inj_test == CRO_COV_TEST_F32 && elem16[r] == p.inj_elem)
          got ^= p.inj_flip;
        t_f32.add(got ^ f32_bits(want_f32[r]), elem16[r]);
      }
    }
    {
      const i32x4 acc = wave_mfma_i8(p.A8 + z, p.B8 + z, CRO_COV_I8_K, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        uint32_t got = (uint32_t)acc[r];
        if (inj_computed && p.inj_test == CRO_COV_TEST_I8 && elem16[r] == p.inj_elem)
          got ^= p.inj_flip;
        t_i8.add(got ^ (uint32_t)want_i8[r], elem16[r]);
      }
    }
    {
      const f32x16 acc = wave_mfma_bf16(p.A16 + z, p.B16 + z, CRO_COV_BF16_K, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        uint32_t got = f32_bits(acc[r]);
        if (inj_computed && p.inj_test == CRO_COV_TEST_BF16 && elem32[r] == p.inj_elem)
          got ^= p.inj_flip;
        t_bf16.add(got ^ f32_bits(want_bf16[r]), elem32[r]);
      }
    }

    // LDS march.  Thread t owns vectors t, t + 256, ...; the verify loop
    // runs on lane 0's vector index, which a wave shares, so all 64 lanes
    // reach every ballot.
    for (uint32_t invert = 0; invert < 2; ++invert) {
      for (uint32_t v = tid; v < n4; v += kBlock) lds4[v] = lds_want(lds_base, v, p.seed, invert);
      __syncthreads();
      if constexpr (kSeams) {
        if (plant && (p.inj_pass == 2 || p.inj_pass == invert)) {
          // vector v is altered by thread (v + 128) % 256, two waves away from
          // the wave that verifies it; only the planted words are stored
          uint32_t* lds1 = reinterpret_cast<uint32_t*>(smem);
          const uint32_t lo = p.inj_elem, hi = p.inj_elem + p.inj_span;  // hi <= lds_words
          for (uint32_t v = ((lo >> 2) & ~(uint32_t)(kBlock - 1)) | (tid ^ 128u);
               (v << 2) < hi; v += kBlock)
            for (uint32_t w = v << 2; w < (v << 2) + 4; ++w)
              if (w >= lo && w < hi) lds1[w] ^= p.inj_flip;
          __syncthreads();
        }
        if (p.dump_out != nullptr && p.dump_pass == invert) {
          uint4* dst = reinterpret_cast<uint4*>(p.dump_out) + (size_t)blockIdx.x * n4;
          for (uint32_t v = tid; v < n4; v += kBlock) dst[v] = lds4[v];
          uint32_t changed = 0;
          for (uint32_t v = n4 + tid; v < n4 + p.guard_vecs; v += kBlock) {
            const uint4 g = lds4[v];
            changed += (g.x != kGuardWord) + (g.y != kGuardWord) + (g.z != kGuardWord) +
                       (g.w != kGuardWord);
          }
          if (changed) atomicAdd(p.guard_bad, changed);
          return;
        }
      }
      for (uint32_t v0 = tid - lane; v0 < n4; v0 += kBlock) {
        const uint32_t v = v0 + lane;
        const uint4 want = lds_want(lds_base, v, p.seed, invert);
        uint4 got = want;  // lanes past the end compare equal
        if (v < n4) got = lds4[v];
        const uint32_t d[4] = {got.x ^ want.x, got.y ^ want.y, got.z ^ want.z,
                               got.w ^ want.w};
        // the same lane and trip in each of the four waves (bits 7:6 of v)
        const bool hit = inj_lds && v < n4 && ((v ^ inj_vec) & ~0xC0u) == 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          t_lds.add(hit && inj_word == (uint32_t)j ? d[j] ^ p.inj_flip : d[j], (v << 2) + j);
      }
      __syncthreads();
    }
  }

  t_f32.reduce();
  t_i8.reduce();
  t_bf16.reduce();
  t_lds.reduce();
  if (lane == 0) {
    CroCoverageRecord rec;
    rec.xcc_id = xcc_id;
    rec.hw_id = hw_id;
    rec.fail_mask = (t_f32.n_bad ? 1u : 0u) | (t_i8.n_bad ? 2u : 0u) |
                    (t_bf16.n_bad ? 4u : 0u) | (t_lds.n_bad ? 8u : 0u);
    rec.n_bad = t_f32.n_bad + t_i8.n_bad + t_bf16.n_bad + t_lds.n_bad;
    const Tally& lead = t_f32.n_bad ? t_f32 : t_i8.n_bad ? t_i8 : t_bf16.n_bad ? t_bf16 : t_lds;
    rec.first_bad = lead.first;
    rec.bits_bad = lead.bits;
    rec.valid = 1;
    rec.reserved = 0;
    p.records[blockIdx.x * kWaves + wave] = rec;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// Per-device cached context (CtxBase, crohost.h): inputs and expected tiles
// are built and uploaded once per device (and again only when the seed
// changes); the record buffer grows on demand.
struct CovCtx : CtxBase {
  int tiles_ready = 0;
  uint32_t seed = 0;
  int cus = 0;
  float *dA32 = nullptr, *dB32 = nullptr, *dE32 = nullptr;
  int8_t *dA8 = nullptr, *dB8 = nullptr;
  int* dE8 = nullptr;
  uint16_t *dA16 = nullptr, *dB16 = nullptr;
  float* dE16 = nullptr;
  // one call's own expected tiles (the caller's, or self-test mode 1's copy
  // with one bit flipped); the cached tiles above stay
  float* dX32 = nullptr;
  int* dX8 = nullptr;
  float* dX16 = nullptr;
  float hE32[CRO_COV_F32_ELEMS];
  int hE8[CRO_COV_I8_ELEMS];
  float hE16[CRO_COV_BF16_ELEMS];
  RecordBuf<CroCoverageRecord> records;
};
CovCtx g_cctx[kMaxDevices];

int upload_tiles(CovCtx* ctx, uint32_t seed, CroComputeResult* out) {
  static float A32[16 * CRO_COV_F32_K], B32[CRO_COV_F32_K * 16];
  static int8_t A8[16 * CRO_COV_I8_K], B8[CRO_COV_I8_K * 16];
  static int Ai[32 * CRO_COV_BF16_K], Bi[CRO_COV_BF16_K * 32];
  static uint16_t A16[32 * CRO_COV_BF16_K], B16[CRO_COV_BF16_K * 32];
  static std::mutex build_mu;  // the statics above are shared by all devices
  std::lock_guard<std::mutex> lock(build_mu);
  cro_cov_make_f32(seed, A32, B32);
  cro_cov_ref_f32(A32, B32, ctx->hE32);
  cro_cov_make_i8(seed, A8, B8);
  cro_cov_ref_i8(A8, B8, ctx->hE8);
  cro_cov_make_bf16(seed, Ai, Bi, A16, B16);
  cro_cov_ref_bf16(Ai, Bi, ctx->hE16);
  CHECK(hipMemcpy(ctx->dA32, A32, sizeof(A32), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(ctx->dB32, B32, sizeof(B32), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(ctx->dE32, ctx->hE32, sizeof(ctx->hE32), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(ctx->dA8, A8, sizeof(A8), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(ctx->dB8, B8, sizeof(B8), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(ctx->dE8, ctx->hE8, sizeof(ctx->hE8), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(ctx->dA16, A16, sizeof(A16), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(ctx->dB16, B16, sizeof(B16), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(ctx->dE16, ctx->hE16, sizeof(ctx->hE16), hipMemcpyHostToDevice));
  ctx->seed = seed;
  ctx->tiles_ready = 1;
  return 0;
}

// The caller's expected tiles of cro_probe_compute_tiles; null = the cached one.
struct CallerTiles {
  const float* e32 = nullptr;
  const int* e8 = nullptr;
  const float* e16 = nullptr;
};

// First use of a device, and the tiles of `seed`; the slot's lock is held.
int prepare(CovCtx* ctx, int device, uint32_t seed, CroComputeResult* out) {
  if (!ctx->ready) {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, device));
    ctx->cus = prop.multiProcessorCount;
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(coverage_kernel<false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               CRO_COV_MAX_LDS_BYTES));
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(coverage_kernel<true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               CRO_COV_MAX_LDS_BYTES));
    CHECK(hipEventCreate(&ctx->e0));
    CHECK(hipEventCreate(&ctx->e1));
    CHECK(hipMalloc(&ctx->dA32, 16 * CRO_COV_F32_K * sizeof(float)));
    CHECK(hipMalloc(&ctx->dB32, CRO_COV_F32_K * 16 * sizeof(float)));
    CHECK(hipMalloc(&ctx->dE32, sizeof(ctx->hE32)));
    CHECK(hipMalloc(&ctx->dA8, 16 * CRO_COV_I8_K));
    CHECK(hipMalloc(&ctx->dB8, CRO_COV_I8_K * 16));
    CHECK(hipMalloc(&ctx->dE8, sizeof(ctx->hE8)));
    CHECK(hipMalloc(&ctx->dA16, 32 * CRO_COV_BF16_K * sizeof(uint16_t)));
    CHECK(hipMalloc(&ctx->dB16, CRO_COV_BF16_K * 32 * sizeof(uint16_t)));
    CHECK(hipMalloc(&ctx->dE16, sizeof(ctx->hE16)));
    CHECK(hipMalloc(&ctx->dX32, sizeof(ctx->hE32)));
    CHECK(hipMalloc(&ctx->dX8, sizeof(ctx->hE8)));
    CHECK(hipMalloc(&ctx->dX16, sizeof(ctx->hE16)));
    ctx->ready = 1;
  }
  if (!ctx->tiles_ready || ctx->seed != seed) {
    ctx->tiles_ready = 0;
    if (upload_tiles(ctx, seed, out) != 0) return -1;
  }
  return 0;
}

// The stage's aggregate as crohost.h's templates call it.
void aggregate(const CroCoverageRecord* records, size_t n, CroCoverageAgg* out) {
  cro_coverage_aggregate(records, n, 0, out);
}

void set_inputs(const CovCtx* ctx, CovParams* p) {
  memset(p, 0, sizeof(*p));
  p->A32 = ctx->dA32;
  p->B32 = ctx->dB32;
  p->E32 = ctx->dE32;
  p->A8 = ctx->dA8;
  p->B8 = ctx->dB8;
  p->E8 = ctx->dE8;
  p->A16 = ctx->dA16;
  p->B16 = ctx->dB16;
  p->E16 = ctx->dE16;
}

int run_compute(int device, const CroComputeOpts* opts, const CallerTiles& tiles,
                CroComputeResult* out, CroCoverageRecord* records_out, int max_records) {
  CroComputeOpts o;
  memset(&o, 0, sizeof(o));
  if (opts) o = *opts;
  if (o.grid_blocks < 0 || o.grid_blocks > kMaxGrid) return bad_arg(out, "grid_blocks");
  if (o.lds_bytes < 0 || o.lds_bytes > CRO_COV_MAX_LDS_BYTES || (o.lds_bytes & 15))
    return bad_arg(out, "lds_bytes must be a multiple of 16, at most 163840");
  if (o.iters < 0 || o.iters > kMaxIters) return bad_arg(out, "iters");
  if (o.max_rounds < 0 || o.max_rounds > kMaxRounds) return bad_arg(out, "max_rounds");
  if (o.min_cu_fraction < 0.0 || o.min_cu_fraction > 1.0) return bad_arg(out, "min_cu_fraction");
  const int lds_bytes = o.lds_bytes ? o.lds_bytes : CRO_COV_MAX_LDS_BYTES;
  const int iters = o.iters ? o.iters : kDefaultIters;
  const int max_rounds = o.max_rounds ? o.max_rounds : kDefaultRounds;
  // the self-test only ever names an element that exists: the host indexes
  // the expected tile with it
  if (o.selftest_mode < 0 || o.selftest_mode > 4) return bad_arg(out, "selftest_mode");
  const bool plant = o.selftest_mode >= 3;  // real LDS stores: the LDS test only
  if (o.selftest_mode) {
    const uint32_t elems[CRO_COV_TESTS] = {CRO_COV_F32_ELEMS, CRO_COV_I8_ELEMS,
                                           CRO_COV_BF16_ELEMS, (uint32_t)lds_bytes / 4};
    if (o.selftest_test < 0 || o.selftest_test >= CRO_COV_TESTS)
      return bad_arg(out, "selftest_test");
    if (o.selftest_bit < 0 || o.selftest_bit > 31) return bad_arg(out, "selftest_bit");
    if (o.selftest_elem >= elems[o.selftest_test]) return bad_arg(out, "selftest_elem");
    if (plant) {
      if (o.selftest_test != CRO_COV_TEST_LDS)
        return bad_arg(out, "selftest_test: modes 3 and 4 plant in LDS");
      if (o.selftest_span < 1 || o.selftest_span > elems[CRO_COV_TEST_LDS] - o.selftest_elem)
        return bad_arg(out, "selftest_span");
      if (o.selftest_pass < 0 || o.selftest_pass > 2) return bad_arg(out, "selftest_pass");
    }
  }

  std::unique_lock<std::mutex> lock;
  CovCtx* ctx = enter_device(g_cctx, device, lock, out->msg, sizeof(out->msg));
  if (ctx == nullptr) return -1;
  if (prepare(ctx, device, o.seed, out) != 0) return -1;
  const int grid = o.grid_blocks ? o.grid_blocks : ctx->cus;
  if (grid < 1) return bad_arg(out, "device reports no compute units");
  const size_t per_round = (size_t)grid * kWaves;
  CHECK(ctx->records.reserve(per_round * (size_t)max_rounds));
  out->cus_expected = ctx->cus;
  out->grid_blocks = grid;
  out->lds_bytes = lds_bytes;
  out->iters = iters;

  CovParams p;
  set_inputs(ctx, &p);
  p.lds_words = (uint32_t)lds_bytes / 4;
  p.iters = (uint32_t)iters;
  p.seed = o.seed;
  p.inj_mode = (uint32_t)o.selftest_mode;
  p.inj_test = (uint32_t)o.selftest_test;
  p.inj_elem = o.selftest_elem;
  p.inj_flip = 1u << (o.selftest_bit & 31);
  p.inj_key = o.selftest_key;
  p.inj_span = o.selftest_span;
  p.inj_pass = (uint32_t)o.selftest_pass;
  // This call's own expected tiles: the caller's, or for self-test mode 1 a
  // copy with one bit of one element flipped.  The kernel sees a pointer.
  const bool flip = o.selftest_mode == 1 && o.selftest_test != CRO_COV_TEST_LDS;
  const auto own_tile = [&](int test, const void* caller, const void* cached, void* dev,
                            size_t bytes) -> hipError_t {
    uint32_t alt[CRO_COV_BF16_ELEMS];
    memcpy(alt, caller ? caller : cached, bytes);
    if (flip && o.selftest_test == test) alt[o.selftest_elem] ^= p.inj_flip;
    return hipMemcpy(dev, alt, bytes, hipMemcpyHostToDevice);
  };
  if (tiles.e32 || (flip && o.selftest_test == CRO_COV_TEST_F32)) {
    CHECK(own_tile(CRO_COV_TEST_F32, tiles.e32, ctx->hE32, ctx->dX32, sizeof(ctx->hE32)));
    p.E32 = ctx->dX32;
  }
  if (tiles.e8 || (flip && o.selftest_test == CRO_COV_TEST_I8)) {
    CHECK(own_tile(CRO_COV_TEST_I8, tiles.e8, ctx->hE8, ctx->dX8, sizeof(ctx->hE8)));
    p.E8 = ctx->dX8;
  }
  if (tiles.e16 || (flip && o.selftest_test == CRO_COV_TEST_BF16)) {
    CHECK(own_tile(CRO_COV_TEST_BF16, tiles.e16, ctx->hE16, ctx->dX16, sizeof(ctx->hE16)));
    p.E16 = ctx->dX16;
  }

  const auto launch = [&](CroCoverageRecord* d_round) {
    p.records = d_round;
    if (plant)
      hipLaunchKernelGGL(coverage_kernel<true>, dim3(grid), dim3(kBlock), (size_t)lds_bytes, 0, p);
    else
      hipLaunchKernelGGL(coverage_kernel<false>, dim3(grid), dim3(kBlock), (size_t)lds_bytes, 0,
                         p);
  };
  if (run_rounds(*ctx, ctx->records.d, ctx->cus, per_round, max_rounds, launch, aggregate, out,
                 records_out, max_records) != 0)
    return -1;
  const CroCoverageAgg& a = out->agg;
  if (a.waves_bad) {
    snprintf(out->failed_test, sizeof(out->failed_test), "%s",
             cro_cov_test_name(a.first_fail_mask));
    snprintf(out->msg, sizeof(out->msg),
             "compute mismatch in %s at xcd=%d se=%d sh=%d cu=%d simd=%d: element %u, "
             "bits 0x%08x; %llu of %llu waves bad on %d CUs",
             out->failed_test, a.xcd, a.se, a.sh, a.cu, a.simd, a.first_bad, a.bits_bad,
             a.waves_bad, a.waves_run, a.cus_bad);
    return -30;
  }
  return coverage_floor(out, ctx->cus, o.min_cu_fraction, -31);
}

int run_lds_dump(int device, int grid_blocks, int lds_bytes, uint32_t seed, int pass,
                 uint32_t plant_elem, uint32_t plant_span, int plant_bit, uint32_t* host_out,
                 unsigned int* guard_bad_out, CroComputeResult* out) {
  if (grid_blocks < 1 || grid_blocks > kMaxDumpGrid) return -10;
  if (lds_bytes < 16 || lds_bytes > CRO_COV_MAX_LDS_BYTES || (lds_bytes & 15)) return -10;
  if (pass < 0 || pass > 1 || host_out == nullptr || guard_bad_out == nullptr) return -10;
  const uint32_t lds_words = (uint32_t)lds_bytes / 4;
  if (plant_span) {
    if (plant_bit < 0 || plant_bit > 31) return -10;
    if (plant_elem >= lds_words || plant_span > lds_words - plant_elem) return -10;
  }
  const bool guarded = lds_bytes <= CRO_COV_MAX_LDS_BYTES - kGuardBytes;

  std::unique_lock<std::mutex> lock;
  CovCtx* ctx = enter_device(g_cctx, device, lock, out->msg, sizeof(out->msg));
  if (ctx == nullptr) return -1;
  if (prepare(ctx, device, seed, out) != 0) return -1;
  CHECK(ctx->records.reserve((size_t)grid_blocks * kWaves));
  const size_t dump_bytes = (size_t)grid_blocks * lds_bytes;
  DevBuf<uint32_t> d_dump;
  DevBuf<unsigned int> d_guard;
  CHECK(d_dump.alloc(dump_bytes));
  CHECK(d_guard.alloc(sizeof(unsigned int)));
  CHECK(hipMemset(d_dump.get(), 0, dump_bytes));
  CHECK(hipMemset(d_guard.get(), 0, sizeof(unsigned int)));

  CovParams p;
  set_inputs(ctx, &p);
  p.records = ctx->records.d;  // the kernel returns before it writes one
  p.lds_words = lds_words;
  p.iters = 1;
  p.seed = seed;
  p.inj_mode = plant_span ? 3u : 0u;
  p.inj_test = CRO_COV_TEST_LDS;
  p.inj_elem = plant_elem;
  p.inj_flip = 1u << (plant_bit & 31);
  p.inj_span = plant_span;
  p.inj_pass = (uint32_t)pass;
  p.dump_out = d_dump.get();
  p.dump_pass = (uint32_t)pass;
  p.guard_vecs = guarded ? kGuardBytes / 16 : 0;
  p.guard_bad = d_guard.get();
  hipLaunchKernelGGL(coverage_kernel<true>, dim3(grid_blocks), dim3(kBlock),
                     (size_t)lds_bytes + (guarded ? kGuardBytes : 0), 0, p);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(host_out, d_dump.get(), dump_bytes, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(guard_bad_out, d_guard.get(), sizeof(unsigned int), hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" int cro_probe_compute_tiles(int device, const struct CroComputeOpts* opts,
                                       const float* e32, const int* e8, const float* e16,
                                       struct CroComputeResult* out,
                                       struct CroCoverageRecord* records_out,
                                       int max_records) {
  clear_result(out, aggregate);
  CallerTiles tiles;
  tiles.e32 = e32;
  tiles.e8 = e8;
  tiles.e16 = e16;
  const double t0 = now_ms();
  out->rc = run_compute(device, opts, tiles, out, records_out, max_records);
  out->t_total_ms = now_ms() - t0;
  return out->rc;
}

extern "C" int cro_probe_compute_records(int device, const struct CroComputeOpts* opts,
                                         struct CroComputeResult* out,
                                         struct CroCoverageRecord* records_out,
                                         int max_records) {
  return cro_probe_compute_tiles(device, opts, nullptr, nullptr, nullptr, out, records_out,
                                 max_records);
}

extern "C" int cro_probe_compute_lds_dump(int device, int grid_blocks, int lds_bytes,
                                          unsigned int seed, int pass,
                                          unsigned int plant_elem, unsigned int plant_span,
                                          int plant_bit, unsigned int* host_out,
                                          unsigned int* guard_bad_out) {
  CroComputeResult res;  // for the HIP error text, which this entry does not return
  clear_result(&res, aggregate);
  return run_lds_dump(device, grid_blocks, lds_bytes, seed, pass, plant_elem, plant_span,
                      plant_bit, host_out, guard_bad_out, &res);
}

extern "C" int cro_probe_compute(int device, const struct CroComputeOpts* opts,
                                 struct CroComputeResult* out) {
  return cro_probe_compute_records(device, opts, out, nullptr, 0);
}

extern "C" int cro_probe_mfma_tile(int device, int kind, const void* A, const void* B,
                                   void* D, int K) {
  if (kind != 1 && kind != 2) return -10;
  const int step = kind == 1 ? 64 : 16;
  if (A == nullptr || B == nullptr || D == nullptr) return -10;
  if (K <= 0 || K > kMaxTileK || K % step != 0) return -10;
  const int rows = kind == 1 ? 16 : 32;
  const size_t esz = kind == 1 ? 1 : 2;
  const size_t in_bytes = (size_t)rows * K * esz, out_bytes = (size_t)rows * rows * 4;
  if (hipSetDevice(device) != hipSuccess) return -1;
  DevBuf<void> dA, dB, dD;
  const auto run = [&]() -> hipError_t {
    TRY(dA.alloc(in_bytes));
    TRY(dB.alloc(in_bytes));
    TRY(dD.alloc(out_bytes));
    TRY(hipMemcpy(dA.get(), A, in_bytes, hipMemcpyHostToDevice));
    TRY(hipMemcpy(dB.get(), B, in_bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(mfma_tile_kernel, dim3(1), dim3(64), 0, 0, kind, dA.get(), dB.get(),
                       dD.get(), K);
    TRY(hipGetLastError());
    return hipMemcpy(D, dD.get(), out_bytes, hipMemcpyDeviceToHost);
  };
  return run() == hipSuccess ? 0 : -1;
}
