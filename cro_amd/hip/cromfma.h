// One wave's matrix products on the gfx950 matrix pipe, and the maps from a
// lane's result registers to tile elements.  Device code shared by the quick
// probe's exact f32 check (probe.hip) and by the coverage kernel and the raw
// tile entry (coverage.hip).
//
// Operand lane maps, lane l of 64:
//   f32 16x16x4   A[l&15][k = l>>4],             B[k = l>>4][l&15]
//   i8  16x16x64  A[l&15][k = 16(l>>4) + j],     B[k = 16(l>>4) + j][l&15]
//                 j = 0..15, byte j&3 of register j>>2 (derived from the
//                 bf16 16x16x32 map; proved bit-exactly on the GPU by the
//                 lane-map tests through cro_probe_mfma_tile)
//   bf16 32x32x16 A[l&31][k = 8(l>>5) + j],      B[k = 8(l>>5) + j][l&31]
// Result maps (dtype-independent): 16x16 register r is row 4(l>>4) + r,
// column l&15; 32x32 register r is row (r&3) + 8(r>>2) + 4(l>>5), column l&31.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

// element index (row * 16 + col) of register r of a 16x16 result
__device__ static inline uint32_t mfma_elem16(uint32_t lane, uint32_t r) {
  return ((lane >> 4) * 4 + r) * 16 + (lane & 15);
}

// element index (row * 32 + col) of register r of a 32x32 result
__device__ static inline uint32_t mfma_elem32(uint32_t lane, uint32_t r) {
  return ((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * 32 + (lane & 31);
}

// K a multiple of 4.  gfx950's f32-input MFMA is bitwise a k-ordered fmaf
// chain, so the host can verify this tile exactly.
__device__ static inline f32x4 wave_mfma_f32(const float* __restrict__ A,
                                             const float* __restrict__ B, int K,
                                             uint32_t lane) {
  const uint32_t rc = lane & 15, kh = lane >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 4) {
    const float a = A[rc * K + (k0 + kh)];
    const float b = B[(k0 + kh) * 16 + rc];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// A rows are 16-byte aligned: K is a multiple of 64 and the base comes from
// hipMalloc.
__device__ static inline i32x4 wave_mfma_i8(const int8_t* __restrict__ A,
                                            const int8_t* __restrict__ B, int K,
                                            uint32_t lane) {
  const uint32_t rc = lane & 15, kh = lane >> 4;
  i32x4 acc = {0, 0, 0, 0};
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int kb = k0 + 16 * (int)kh;
    const i32x4 a = *reinterpret_cast<const i32x4*>(A + rc * K + kb);
    i32x4 b;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t w = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        w |= (uint32_t)(uint8_t)B[(kb + 4 * q + j) * 16 + rc] << (8 * j);
      b[q] = (int)w;
    }
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
  }
  return acc;
}

__device__ static inline f32x16 wave_mfma_bf16(const uint16_t* __restrict__ A,
                                               const uint16_t* __restrict__ B, int K,
                                               uint32_t lane) {
  const uint32_t rc = lane & 31, h = lane >> 5;
  f32x16 acc = {};
  for (int k0 = 0; k0 < K; k0 += 16) {
    const int kb = k0 + 8 * (int)h;
    const u16x8 au = *reinterpret_cast<const u16x8*>(A + rc * K + kb);
    u16x8 bu;
#pragma unroll
    for (int j = 0; j < 8; ++j) bu[j] = B[(kb + j) * 32 + rc];
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, au),
                                                  __builtin_bit_cast(bf16x8, bu), acc, 0, 0,
                                                  0);
  }
  return acc;
}
