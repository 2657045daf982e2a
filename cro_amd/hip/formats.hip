// cro_amd gfx950 matrix-format probe stage: exact checks of the f16, fp8, bf8,
// block-scaled fp8 / fp6 / fp4 and f64 matrix paths on every CU and SIMD, with
// fault location.
//
// The compute-coverage stage (coverage.hip) checks the f32, i8 and bf16
// instructions; nothing there decodes a narrow operand format, applies an
// E8M0 scale or runs the f64 matrix path, whose result map differs.  This
// stage follows its shape: one 256-thread workgroup per CU (a CU's whole
// dynamic LDS is requested for placement only and never touched), four waves,
// one per SIMD, and each wave computes the seven products of croformats.h
// `iters` times.  Each lane compares its own result registers bit for bit
// with an expected tile built on the host; mismatches are counted per wave
// with a 64-lane ballot and popcount, the OR of bad bits and the lowest bad
// element are reduced with shuffles, each wave reads where it ran (XCC_ID,
// HW_ID) and lane 0 writes one CroFormatsRecord.  Workgroups are independent:
// no inter-workgroup communication, no spin, no LDS traffic, no atomics.  The
// host aggregates the records and launches the same grid again, a bounded
// number of times, while some CU or SIMD is still unseen.
//
// The lane, packing and scale maps the wave code below relies on are written
// at the head of croformats.h; cro_formats_tile runs one wave of the same
// code on caller data, which is how the tests prove them.
//
// A library of its own (libcroformats.so): host plumbing from crohost.h, the
// f32 result maps from cromfma.h.

#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>

#include "croformats.h"
#include "crohost.h"
#include "cromfma.h"

namespace {

constexpr int kWaves = kBlock / 64;
// ≈0.008 ms per repeat on an MI355X: 64 is the largest power of two that keeps
// the stage no more expensive than the compute-coverage stage's default
// (0.52 ms against 0.57 ms, profiles/formats_probe_mi355x.md)
constexpr int kDefaultIters = 64;
constexpr int kDefaultRounds = 4;
constexpr int kMaxRounds = 64;
constexpr int kMaxGrid = 1 << 16;
constexpr int kMaxIters = 1 << 16;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

// element index (row * 16 + col) of register r of the f64 16x16 result
__device__ inline uint32_t mfma_elem16_f64(uint32_t lane, uint32_t r) {
  return ((lane >> 4) + 4 * r) * 16 + (lane & 15);
}

// ---------------------------------------------------------------------------
// one wave's products; A and B are K-contiguous rows, packed (croformats.h)
// ---------------------------------------------------------------------------

// rows are 16-byte aligned: K is a multiple of 32 and the base comes from hipMalloc
__device__ inline f32x4 wave_f16(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                 int K, uint32_t lane) {
  const uint32_t rc = lane & 15, kh = lane >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 32) {
    const size_t off = ((size_t)rc * K + k0 + 8 * kh) * 2;
    const f16x8 a = *reinterpret_cast<const f16x8*>(A + off);
    const f16x8 b = *reinterpret_cast<const f16x8*>(B + off);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
  }
  return acc;
}

__device__ inline f32x4 wave_fp8(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                 int K, uint32_t lane) {
  const uint32_t rc = lane & 15, kh = lane >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 32) {
    const size_t off = (size_t)rc * K + k0 + 8 * kh;
    const long a = *reinterpret_cast<const long*>(A + off);
    const long b = *reinterpret_cast<const long*>(B + off);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, acc, 0, 0, 0);
  }
  return acc;
}

__device__ inline f32x16 wave_bf8(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                  int K, uint32_t lane) {
  const uint32_t rc = lane & 31, h = lane >> 5;
  f32x16 acc = {};
  for (int k0 = 0; k0 < K; k0 += 16) {
    const size_t off = (size_t)rc * K + k0 + 8 * h;
    const long a = *reinterpret_cast<const long*>(A + off);
    const long b = *reinterpret_cast<const long*>(B + off);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf8_bf8(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// The 32 elements of K block g of one row as the scaled instruction's 8-int
// operand: 8, 6 or 4 registers hold data, the rest are zero.  FMT is the
// cbsz / blgp code.  4-byte aligned: a block is 32, 24 or 16 bytes.
template <int FMT>
__device__ inline i32x8 load_block(const uint8_t* __restrict__ row, int g) {
  constexpr int kRegs = FMT <= 1 ? 8 : FMT <= 3 ? 6 : 4;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(row + (size_t)g * (kRegs * 4));
  i32x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < kRegs; ++q) v[q] = (int)src[q];
  return v;
}

// The scale register of a lane: its scale in byte `sel`, three other valid
// scales, all different from it, in the other bytes, so a wrong byte select
// gives wrong data rather than NaN.
__device__ inline int scale_reg(uint32_t s, int sel) {
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t other = (s + 37u * (1u + (uint32_t)((j - sel) & 3))) % 255u;
    w |= (j == sel ? s : other) << (8 * j);
  }
  return (int)w;
}

// One lane's operand of the 16x16x128 form for the K blocks g0 .. g0+3, lane
// group kb = l>>4.  6- and 4-bit formats: the 32 contiguous k of block
// g0 + kb.  8-bit formats: registers 0..3 hold k = 16 kb + j and registers
// 4..7 hold k = 64 + 16 kb + j, j = 0..15, of those 128; the scale of lane
// group kb still belongs to block g0 + kb, whose 32 elements sit in registers
// 0..3 (kb < 2) or 4..7 of two other lane groups.
template <int FMT>
__device__ inline i32x8 load_operand16(const uint8_t* __restrict__ row, int g0, uint32_t kb) {
  if constexpr (FMT <= 1) {
    const uint32_t* lo = reinterpret_cast<const uint32_t*>(row + 32 * g0 + 16 * kb);
    const uint32_t* hi = reinterpret_cast<const uint32_t*>(row + 32 * g0 + 64 + 16 * kb);
    i32x8 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[q] = (int)lo[q];
      v[4 + q] = (int)hi[q];
    }
    return v;
  } else {
    return load_block<FMT>(row, g0 + (int)kb);
  }
}

// 16x16x128: row / column l&15, lane group l>>4.  K a multiple of 128.
template <int FA, int FB, int OSA, int OSB>
__device__ inline f32x4 wave_mx16(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                  const uint8_t* __restrict__ SA,
                                  const uint8_t* __restrict__ SB, int K, uint32_t lane) {
  constexpr int kBitsA = FA <= 1 ? 8 : FA <= 3 ? 6 : 4, kBitsB = FB <= 1 ? 8 : FB <= 3 ? 6 : 4;
  const uint32_t rc = lane & 15, kb = lane >> 4;
  const int G = K / 32;
  const uint8_t* rowA = A + (size_t)rc * K * kBitsA / 8;
  const uint8_t* rowB = B + (size_t)rc * K * kBitsB / 8;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int g0 = 0; g0 < G; g0 += 4) {
    const int g = g0 + (int)kb;
    const i32x8 a = load_operand16<FA>(rowA, g0, kb);
    const i32x8 b = load_operand16<FB>(rowB, g0, kb);
    const int sa = scale_reg(SA[rc * G + g], OSA);
    const int sb = scale_reg(SB[rc * G + g], OSB);
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, FA, FB, OSA, sa, OSB, sb);
  }
  return acc;
}

// 32x32x64: lane l holds block l>>5 of row / column l&31.  K a multiple of 64.
// 6- and 4-bit formats only: the 8-bit lane map of this shape is not proved.
template <int FA, int FB, int OSA, int OSB>
__device__ inline f32x16 wave_mx32(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                   const uint8_t* __restrict__ SA,
                                   const uint8_t* __restrict__ SB, int K, uint32_t lane) {
  static_assert(FA > 1 && FB > 1, "8-bit operands of the 32x32x64 form: lane map not proved");
  constexpr int kBitsA = FA <= 1 ? 8 : FA <= 3 ? 6 : 4, kBitsB = FB <= 1 ? 8 : FB <= 3 ? 6 : 4;
  const uint32_t rc = lane & 31, kb = lane >> 5;
  const int G = K / 32;
  const uint8_t* rowA = A + (size_t)rc * K * kBitsA / 8;
  const uint8_t* rowB = B + (size_t)rc * K * kBitsB / 8;
  f32x16 acc = {};
  for (int g0 = 0; g0 < G; g0 += 2) {
    const int g = g0 + (int)kb;
    const i32x8 a = load_block<FA>(rowA, g);
    const i32x8 b = load_block<FB>(rowB, g);
    const int sa = scale_reg(SA[rc * G + g], OSA);
    const int sb = scale_reg(SB[rc * G + g], OSB);
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, FA, FB, OSA, sa, OSB, sb);
  }
  return acc;
}

__device__ inline f64x4 wave_f64(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                 int K, uint32_t lane) {
  const uint32_t rc = lane & 15, kh = lane >> 4;
  const double* a64 = reinterpret_cast<const double*>(A);
  const double* b64 = reinterpret_cast<const double*>(B);
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < K; k0 += 4) {
    const double a = a64[(size_t)rc * K + k0 + kh];
    const double b = b64[(size_t)rc * K + k0 + kh];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// ---------------------------------------------------------------------------
// raw tile entry: one wave of the products above, stored through the result maps
// ---------------------------------------------------------------------------

struct TileArgs {
  const uint8_t *A, *B, *SA, *SB;
  void* D;
  int K;
};

template <int TEST, int OSA, int OSB>
__global__ __launch_bounds__(64) void tile_kernel(TileArgs t) {
  const uint32_t lane = threadIdx.x;  // exactly one wave of 64
  float* D32 = (float*)t.D;
  if constexpr (TEST == CRO_FMT_TEST_F16) {
    const f32x4 acc = wave_f16(t.A, t.B, t.K, lane);
    for (int r = 0; r < 4; ++r) D32[mfma_elem16(lane, r)] = acc[r];
  } else if constexpr (TEST == CRO_FMT_TEST_FP8) {
    const f32x4 acc = wave_fp8(t.A, t.B, t.K, lane);
    for (int r = 0; r < 4; ++r) D32[mfma_elem16(lane, r)] = acc[r];
  } else if constexpr (TEST == CRO_FMT_TEST_BF8) {
    const f32x16 acc = wave_bf8(t.A, t.B, t.K, lane);
    for (int r = 0; r < 16; ++r) D32[mfma_elem32(lane, r)] = acc[r];
  } else if constexpr (TEST == CRO_FMT_TEST_MX_FP8) {
    const f32x4 acc =
        wave_mx16<CRO_FMT_E4M3, CRO_FMT_E5M2, OSA, OSB>(t.A, t.B, t.SA, t.SB, t.K, lane);
    for (int r = 0; r < 4; ++r) D32[mfma_elem16(lane, r)] = acc[r];
  } else if constexpr (TEST == CRO_FMT_TEST_MX_FP6) {
    const f32x16 acc =
        wave_mx32<CRO_FMT_E2M3, CRO_FMT_E3M2, OSA, OSB>(t.A, t.B, t.SA, t.SB, t.K, lane);
    for (int r = 0; r < 16; ++r) D32[mfma_elem32(lane, r)] = acc[r];
  } else if constexpr (TEST == CRO_FMT_TEST_MX_FP4) {
    const f32x4 acc =
        wave_mx16<CRO_FMT_E2M1, CRO_FMT_E2M1, OSA, OSB>(t.A, t.B, t.SA, t.SB, t.K, lane);
    for (int r = 0; r < 4; ++r) D32[mfma_elem16(lane, r)] = acc[r];
  } else {
    const f64x4 acc = wave_f64(t.A, t.B, t.K, lane);
    for (int r = 0; r < 4; ++r) ((double*)t.D)[mfma_elem16_f64(lane, r)] = acc[r];
  }
}

template <int TEST, int OSA, int OSB>
void launch_tile(const TileArgs& t) {
  hipLaunchKernelGGL((tile_kernel<TEST, OSA, OSB>), dim3(1), dim3(64), 0, 0, t);
}

template <int TEST, int OSA>
void launch_tile_b(int osb, const TileArgs& t) {
  switch (osb) {
    case 0: return launch_tile<TEST, OSA, 0>(t);
    case 1: return launch_tile<TEST, OSA, 1>(t);
    case 2: return launch_tile<TEST, OSA, 2>(t);
    default: return launch_tile<TEST, OSA, 3>(t);
  }
}

template <int TEST>
void launch_tile_ab(int osa, int osb, const TileArgs& t) {
  switch (osa) {
    case 0: return launch_tile_b<TEST, 0>(osb, t);
    case 1: return launch_tile_b<TEST, 1>(osb, t);
    case 2: return launch_tile_b<TEST, 2>(osb, t);
    default: return launch_tile_b<TEST, 3>(osb, t);
  }
}

// ---------------------------------------------------------------------------
// stage kernel
// ---------------------------------------------------------------------------

struct FmtParams {
  const uint8_t* A[CRO_FMT_TESTS];
  const uint8_t* B[CRO_FMT_TESTS];
  const uint8_t* SA[CRO_FMT_TESTS];  // null for the checks without scales
  const uint8_t* SB[CRO_FMT_TESTS];
  const uint32_t* E[CRO_FMT_TESTS];  // expected tiles (cro_fmt_expected)
  CroFormatsRecord* records;         // this round's grid_blocks * 4 records
  uint32_t iters;
  uint32_t inj_mode;  // self-test, see croformats.h
  uint32_t inj_test;
  uint32_t inj_elem;
  uint32_t inj_key;
  uint64_t inj_flip;  // 1 << selftest_bit
};

// What one wave found in one check.  n_bad is wave-uniform (ballot counts);
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

// a lane's N f32 result registers against its N expected words
template <int N, class Acc>
__device__ inline void check_f32(Tally& t, const Acc& acc, const uint32_t (&want)[N],
                                 const uint32_t (&elem)[N], bool inject, uint32_t inj_elem,
                                 uint32_t flip) {
#pragma unroll
  for (int r = 0; r < N; ++r) {
    uint32_t got = f32_bits(acc[r]);
    if (inject && elem[r] == inj_elem) got ^= flip;
    t.add(got ^ want[r], elem[r]);
  }
}

__global__ __launch_bounds__(kBlock) void formats_kernel(FmtParams p) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t xcc_id, hw_id;  // for the report only
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
  // self-test mode 2 flips computed values on the waves of one CU; mode 1 is
  // done on the host
  const bool inj = p.inj_mode == 2 && cro_cov_cu_key(xcc_id, hw_id) == p.inj_key;
  const uint32_t flip32 = (uint32_t)p.inj_flip;

  // the elements this lane holds, and what it expects there
  uint32_t elem16[4], elem32[16], elem64[4];
  uint32_t want_f16[4], want_fp8[4], want_bf8[16], want_mx8[4], want_mx6[16], want_mx4[4];
  uint64_t want_f64[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    elem16[r] = mfma_elem16(lane, r);
    elem64[r] = mfma_elem16_f64(lane, r);
    want_f16[r] = p.E[CRO_FMT_TEST_F16][elem16[r]];
    want_fp8[r] = p.E[CRO_FMT_TEST_FP8][elem16[r]];
    want_mx8[r] = p.E[CRO_FMT_TEST_MX_FP8][elem16[r]];
    want_mx4[r] = p.E[CRO_FMT_TEST_MX_FP4][elem16[r]];
    want_f64[r] = (uint64_t)p.E[CRO_FMT_TEST_F64][2 * elem64[r]] |
                  ((uint64_t)p.E[CRO_FMT_TEST_F64][2 * elem64[r] + 1] << 32);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    elem32[r] = mfma_elem32(lane, r);
    want_bf8[r] = p.E[CRO_FMT_TEST_BF8][elem32[r]];
    want_mx6[r] = p.E[CRO_FMT_TEST_MX_FP6][elem32[r]];
  }

  Tally t[CRO_FMT_TESTS];
  for (uint32_t it = 0; it < p.iters; ++it) {
    // an offset of zero the compiler cannot see through: the products are
    // recomputed, operands reloaded, in every iteration
    uint32_t z = 0;
    asm volatile("" : "+v"(z));
    const auto in = [&](const uint8_t* const (&ptrs)[CRO_FMT_TESTS], int test) {
      return ptrs[test] + z;
    };
    {
      constexpr int T = CRO_FMT_TEST_F16;
      const f32x4 acc = wave_f16(in(p.A, T), in(p.B, T), cro_fmt_k(T), lane);
      check_f32<4>(t[T], acc, want_f16, elem16, inj && p.inj_test == T, p.inj_elem, flip32);
    }
    {
      constexpr int T = CRO_FMT_TEST_FP8;
      const f32x4 acc = wave_fp8(in(p.A, T), in(p.B, T), cro_fmt_k(T), lane);
      check_f32<4>(t[T], acc, want_fp8, elem16, inj && p.inj_test == T, p.inj_elem, flip32);
    }
    {
      constexpr int T = CRO_FMT_TEST_BF8;
      const f32x16 acc = wave_bf8(in(p.A, T), in(p.B, T), cro_fmt_k(T), lane);
      check_f32<16>(t[T], acc, want_bf8, elem32, inj && p.inj_test == T, p.inj_elem, flip32);
    }
    {
      constexpr int T = CRO_FMT_TEST_MX_FP8;
      const f32x4 acc =
          wave_mx16<CRO_FMT_E4M3, CRO_FMT_E5M2, CRO_FMT_MX_FP8_SEL_A, CRO_FMT_MX_FP8_SEL_B>(
              in(p.A, T), in(p.B, T), in(p.SA, T), in(p.SB, T), cro_fmt_k(T), lane);
      check_f32<4>(t[T], acc, want_mx8, elem16, inj && p.inj_test == T, p.inj_elem, flip32);
    }
    {
      constexpr int T = CRO_FMT_TEST_MX_FP6;
      const f32x16 acc =
          wave_mx32<CRO_FMT_E2M3, CRO_FMT_E3M2, CRO_FMT_MX_FP6_SEL_A, CRO_FMT_MX_FP6_SEL_B>(
              in(p.A, T), in(p.B, T), in(p.SA, T), in(p.SB, T), cro_fmt_k(T), lane);
      check_f32<16>(t[T], acc, want_mx6, elem32, inj && p.inj_test == T, p.inj_elem, flip32);
    }
    {
      constexpr int T = CRO_FMT_TEST_MX_FP4;
      const f32x4 acc =
          wave_mx16<CRO_FMT_E2M1, CRO_FMT_E2M1, CRO_FMT_MX_FP4_SEL_A, CRO_FMT_MX_FP4_SEL_B>(
              in(p.A, T), in(p.B, T), in(p.SA, T), in(p.SB, T), cro_fmt_k(T), lane);
      check_f32<4>(t[T], acc, want_mx4, elem16, inj && p.inj_test == T, p.inj_elem, flip32);
    }
    {
      constexpr int T = CRO_FMT_TEST_F64;
      const f64x4 acc = wave_f64(in(p.A, T), in(p.B, T), cro_fmt_k(T), lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        uint64_t got = __builtin_bit_cast(uint64_t, (double)acc[r]);
        if (inj && p.inj_test == T && elem64[r] == p.inj_elem) got ^= p.inj_flip;
        const uint64_t diff = got ^ want_f64[r];
        t[T].add((uint32_t)diff | (uint32_t)(diff >> 32), elem64[r]);
      }
    }
  }

  uint32_t fail_mask = 0, n_bad = 0, first_bad = ~0u, bits_bad = 0;
#pragma unroll
  for (int k = CRO_FMT_TESTS - 1; k >= 0; --k) {
    t[k].reduce();
    if (t[k].n_bad) {  // the lowest failing check leads
      fail_mask |= 1u << k;
      n_bad += t[k].n_bad;
      first_bad = t[k].first;
      bits_bad = t[k].bits;
    }
  }
  if (lane == 0) {
    CroFormatsRecord rec;
    rec.xcc_id = xcc_id;
    rec.hw_id = hw_id;
    rec.fail_mask = fail_mask;
    rec.n_bad = n_bad;
    rec.first_bad = first_bad;
    rec.bits_bad = bits_bad;
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
struct FmtCtx : CtxBase {
  int tiles_ready = 0;
  uint32_t seed = 0;
  int cus = 0;
  uint8_t *dA[CRO_FMT_TESTS] = {}, *dB[CRO_FMT_TESTS] = {};
  uint8_t *dSA[CRO_FMT_TESTS] = {}, *dSB[CRO_FMT_TESTS] = {};
  uint32_t* dE[CRO_FMT_TESTS] = {};
  // self-test mode 1's copy of one expected tile with one bit flipped; the
  // cached tiles above stay
  uint32_t* dX = nullptr;
  uint32_t* dX2 = nullptr;  // selftest_also's
  uint32_t hE[CRO_FMT_TESTS][2 * CRO_FMT_MAX_ELEMS];
  RecordBuf<CroFormatsRecord> records;
};
FmtCtx g_fctx[kMaxDevices];

size_t packed_bytes(int test, int a_side) {
  const CroFmtTestDesc* d = cro_fmt_test(test);
  return (size_t)d->m * cro_fmt_row_bytes(a_side ? d->fmt_a : d->fmt_b, d->k);
}

size_t expected_bytes(int test) {
  return (size_t)cro_fmt_elems(test) * (test == CRO_FMT_TEST_F64 ? 8 : 4);
}

int upload_tiles(FmtCtx* ctx, uint32_t seed, CroFormatsResult* out) {
  static CroFmtInputs in;
  static std::mutex build_mu;  // the static above is shared by all devices
  std::lock_guard<std::mutex> lock(build_mu);
  for (int t = 0; t < CRO_FMT_TESTS; ++t) {
    const CroFmtTestDesc* d = cro_fmt_test(t);
    cro_fmt_make(t, seed, &in);
    cro_fmt_expected(&in, ctx->hE[t]);
    CHECK(hipMemcpy(ctx->dA[t], in.packed_a, packed_bytes(t, 1), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(ctx->dB[t], in.packed_b, packed_bytes(t, 0), hipMemcpyHostToDevice));
    if (d->scale_base_a) {
      const size_t ns = (size_t)d->m * (d->k / 32);
      CHECK(hipMemcpy(ctx->dSA[t], in.scale_a, ns, hipMemcpyHostToDevice));
      CHECK(hipMemcpy(ctx->dSB[t], in.scale_b, ns, hipMemcpyHostToDevice));
    }
    CHECK(hipMemcpy(ctx->dE[t], ctx->hE[t], expected_bytes(t), hipMemcpyHostToDevice));
  }
  ctx->seed = seed;
  ctx->tiles_ready = 1;
  return 0;
}

// First use of a device, and the tiles of `seed`; the slot's lock is held.
int prepare(FmtCtx* ctx, int device, uint32_t seed, CroFormatsResult* out) {
  if (!ctx->ready) {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, device));
    ctx->cus = prop.multiProcessorCount;
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(formats_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               CRO_COV_MAX_LDS_BYTES));
    CHECK(hipEventCreate(&ctx->e0));
    CHECK(hipEventCreate(&ctx->e1));
    for (int t = 0; t < CRO_FMT_TESTS; ++t) {
      const CroFmtTestDesc* d = cro_fmt_test(t);
      CHECK(hipMalloc(&ctx->dA[t], packed_bytes(t, 1)));
      CHECK(hipMalloc(&ctx->dB[t], packed_bytes(t, 0)));
      if (d->scale_base_a) {
        CHECK(hipMalloc(&ctx->dSA[t], (size_t)d->m * (d->k / 32)));
        CHECK(hipMalloc(&ctx->dSB[t], (size_t)d->m * (d->k / 32)));
      }
      CHECK(hipMalloc(&ctx->dE[t], expected_bytes(t)));
    }
    CHECK(hipMalloc(&ctx->dX, sizeof(ctx->hE[0])));
    CHECK(hipMalloc(&ctx->dX2, sizeof(ctx->hE[0])));
    ctx->ready = 1;
  }
  if (!ctx->tiles_ready || ctx->seed != seed) {
    ctx->tiles_ready = 0;
    if (upload_tiles(ctx, seed, out) != 0) return -1;
  }
  return 0;
}

int run_formats(int device, const CroFormatsOpts* opts, CroFormatsResult* out,
                CroFormatsRecord* records_out, int max_records) {
  CroFormatsOpts o;
  memset(&o, 0, sizeof(o));
  if (opts) o = *opts;
  if (o.grid_blocks < 0 || o.grid_blocks > kMaxGrid) return bad_arg(out, "grid_blocks");
  if (o.iters < 0 || o.iters > kMaxIters) return bad_arg(out, "iters");
  if (o.max_rounds < 0 || o.max_rounds > kMaxRounds) return bad_arg(out, "max_rounds");
  if (!(o.min_cu_fraction >= 0.0 && o.min_cu_fraction <= 1.0))
    return bad_arg(out, "min_cu_fraction");
  const int iters = o.iters ? o.iters : kDefaultIters;
  const int max_rounds = o.max_rounds ? o.max_rounds : kDefaultRounds;
  // the self-test only ever names an element that exists: the host indexes
  // the expected tile with it
  if (o.selftest_mode < 0 || o.selftest_mode > 2) return bad_arg(out, "selftest_mode");
  if (o.selftest_mode) {
    if (o.selftest_test < 0 || o.selftest_test >= CRO_FMT_TESTS)
      return bad_arg(out, "selftest_test");
    const int top_bit = o.selftest_test == CRO_FMT_TEST_F64 ? 63 : 31;
    if (o.selftest_bit < 0 || o.selftest_bit > top_bit) return bad_arg(out, "selftest_bit");
    if (o.selftest_elem >= (uint32_t)cro_fmt_elems(o.selftest_test))
      return bad_arg(out, "selftest_elem");
    if (o.selftest_also) {
      const int t2 = o.selftest_also - 1;
      if (o.selftest_mode != 1 || t2 < 0 || t2 >= CRO_FMT_TESTS || t2 == o.selftest_test ||
          o.selftest_elem + 1 >= (uint32_t)cro_fmt_elems(t2) ||
          (t2 != CRO_FMT_TEST_F64 && o.selftest_bit > 31))
        return bad_arg(out, "selftest_also");
    }
  } else if (o.selftest_also) {
    return bad_arg(out, "selftest_also");
  }

  std::unique_lock<std::mutex> lock;
  FmtCtx* ctx = enter_device(g_fctx, device, lock, out->msg, sizeof(out->msg));
  if (ctx == nullptr) return -1;
  if (prepare(ctx, device, o.seed, out) != 0) return -1;
  const int grid = o.grid_blocks ? o.grid_blocks : ctx->cus;
  if (grid < 1) return bad_arg(out, "device reports no compute units");
  const size_t per_round = (size_t)grid * kWaves;
  CHECK(ctx->records.reserve(per_round * (size_t)max_rounds));
  out->cus_expected = ctx->cus;
  out->grid_blocks = grid;
  out->iters = iters;

  FmtParams p;
  memset(&p, 0, sizeof(p));
  for (int t = 0; t < CRO_FMT_TESTS; ++t) {
    p.A[t] = ctx->dA[t];
    p.B[t] = ctx->dB[t];
    p.SA[t] = ctx->dSA[t];
    p.SB[t] = ctx->dSB[t];
    p.E[t] = ctx->dE[t];
  }
  p.iters = (uint32_t)iters;
  p.inj_mode = (uint32_t)o.selftest_mode;
  p.inj_test = (uint32_t)o.selftest_test;
  p.inj_elem = o.selftest_elem;
  p.inj_key = o.selftest_key;
  p.inj_flip = 1ull << (o.selftest_bit & 63);
  if (o.selftest_mode == 1) {
    // this call's own expected tile: a copy with one bit of one element flipped
    const auto flipped = [&](int t, uint32_t elem, uint32_t* dev) -> hipError_t {
      std::vector<uint32_t> alt(ctx->hE[t], ctx->hE[t] + expected_bytes(t) / 4);
      if (t == CRO_FMT_TEST_F64)
        alt[2 * elem + (o.selftest_bit >> 5)] ^= 1u << (o.selftest_bit & 31);
      else
        alt[elem] ^= 1u << o.selftest_bit;
      p.E[t] = dev;
      return hipMemcpy(dev, alt.data(), expected_bytes(t), hipMemcpyHostToDevice);
    };
    CHECK(flipped(o.selftest_test, o.selftest_elem, ctx->dX));
    if (o.selftest_also) CHECK(flipped(o.selftest_also - 1, o.selftest_elem + 1, ctx->dX2));
  }

  const auto launch = [&](CroFormatsRecord* d_round) {
    p.records = d_round;
    hipLaunchKernelGGL(formats_kernel, dim3(grid), dim3(kBlock), (size_t)CRO_COV_MAX_LDS_BYTES, 0,
                       p);
  };
  if (run_rounds(*ctx, ctx->records.d, ctx->cus, per_round, max_rounds, launch,
                 cro_formats_aggregate, out, records_out, max_records) != 0)
    return -1;
  const CroFormatsAgg& a = out->agg;
  if (a.waves_bad) {
    snprintf(out->failed_test, sizeof(out->failed_test), "%s",
             cro_fmt_test_name(a.first_fail_mask));
    snprintf(out->msg, sizeof(out->msg),
             "format mismatch in %s at xcd=%d se=%d sh=%d cu=%d simd=%d: element %u, "
             "bits 0x%08x; %llu of %llu waves bad on %d CUs",
             out->failed_test, a.xcd, a.se, a.sh, a.cu, a.simd, a.first_bad, a.bits_bad,
             a.waves_bad, a.waves_run, a.cus_bad);
    return -32;
  }
  return coverage_floor(out, ctx->cus, o.min_cu_fraction, -33);
}

}  // namespace

extern "C" int cro_formats_run_records(int device, const struct CroFormatsOpts* opts,
                                       struct CroFormatsResult* out,
                                       struct CroFormatsRecord* records_out, int max_records) {
  clear_result(out, cro_formats_aggregate);
  const double t0 = now_ms();
  out->rc = run_formats(device, opts, out, records_out, max_records);
  out->t_total_ms = now_ms() - t0;
  return out->rc;
}

extern "C" int cro_formats_run(int device, const struct CroFormatsOpts* opts,
                               struct CroFormatsResult* out) {
  return cro_formats_run_records(device, opts, out, nullptr, 0);
}

extern "C" int cro_formats_tile(int device, int test, int op_sel_a, int op_sel_b, const void* A,
                                const void* B, const unsigned char* scale_a,
                                const unsigned char* scale_b, void* D, int K) {
  if (test < 0 || test >= CRO_FMT_TESTS) return -10;
  const CroFmtTestDesc* d = cro_fmt_test(test);
  const bool scaled = d->scale_base_a != 0;
  if (A == nullptr || B == nullptr || D == nullptr) return -10;
  if (K <= 0 || K > CRO_FMT_MAX_TILE_K || K % d->kstep != 0) return -10;
  if (op_sel_a < 0 || op_sel_a > 3 || op_sel_b < 0 || op_sel_b > 3) return -10;
  if (scaled ? (scale_a == nullptr || scale_b == nullptr) : (op_sel_a || op_sel_b)) return -10;
  const size_t a_bytes = (size_t)d->m * cro_fmt_row_bytes(d->fmt_a, K);
  const size_t b_bytes = (size_t)d->m * cro_fmt_row_bytes(d->fmt_b, K);
  const size_t s_bytes = scaled ? (size_t)d->m * (K / 32) : 0;
  const size_t out_bytes = (size_t)d->m * d->m * (test == CRO_FMT_TEST_F64 ? 8 : 4);
  if (hipSetDevice(device) != hipSuccess) return -1;
  DevBuf<uint8_t> dA, dB, dSA, dSB;
  DevBuf<void> dD;
  const auto run = [&]() -> hipError_t {
    TRY(dA.alloc(a_bytes));
    TRY(dB.alloc(b_bytes));
    TRY(dD.alloc(out_bytes));
    TRY(hipMemcpy(dA.get(), A, a_bytes, hipMemcpyHostToDevice));
    TRY(hipMemcpy(dB.get(), B, b_bytes, hipMemcpyHostToDevice));
    if (scaled) {
      TRY(dSA.alloc(s_bytes));
      TRY(dSB.alloc(s_bytes));
      TRY(hipMemcpy(dSA.get(), scale_a, s_bytes, hipMemcpyHostToDevice));
      TRY(hipMemcpy(dSB.get(), scale_b, s_bytes, hipMemcpyHostToDevice));
    }
    TileArgs t = {dA.get(), dB.get(), dSA.get(), dSB.get(), dD.get(), K};
    switch (test) {
      case CRO_FMT_TEST_F16: launch_tile<CRO_FMT_TEST_F16, 0, 0>(t); break;
      case CRO_FMT_TEST_FP8: launch_tile<CRO_FMT_TEST_FP8, 0, 0>(t); break;
      case CRO_FMT_TEST_BF8: launch_tile<CRO_FMT_TEST_BF8, 0, 0>(t); break;
      case CRO_FMT_TEST_MX_FP8: launch_tile_ab<CRO_FMT_TEST_MX_FP8>(op_sel_a, op_sel_b, t); break;
      case CRO_FMT_TEST_MX_FP6: launch_tile_ab<CRO_FMT_TEST_MX_FP6>(op_sel_a, op_sel_b, t); break;
      case CRO_FMT_TEST_MX_FP4: launch_tile_ab<CRO_FMT_TEST_MX_FP4>(op_sel_a, op_sel_b, t); break;
      default: launch_tile<CRO_FMT_TEST_F64, 0, 0>(t); break;
    }
    TRY(hipGetLastError());
    return hipMemcpy(D, dD.get(), out_bytes, hipMemcpyDeviceToHost);
  };
  return run() == hipSuccess ? 0 : -1;
}
