// Address-dependent data pattern for the deep (data-integrity) probe.
//
// One definition shared by the device kernels (integrity.hip), the host
// side of the link stages and the host-only parity test, so "what the GPU
// wrote" and "what the host expects" cannot drift apart.  Plain C++: a host
// compiler without HIP can include it (the 16-byte vector form at the end is
// for hipcc only; coverage.hip's LDS march uses it too).
//
// The 32-bit word at global word index w (64-bit) under a 32-bit seed:
//
//   x  = (uint32)w ^ seed
//   x += (uint32)(w >> 32) * 0x9E3779B9
//   x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
//
// The final mix (the murmur3 finaliser) is a bijection on 32 bits, and
// within one 2^32-word (16 GiB) window the high half of w is constant, so
// the input to the mix is itself a bijection of the low half.  No two
// addresses of such a window hold the same value: a store that lands on an
// aliased address is therefore always seen by the verify of the address it
// overwrote.  Pass 0 holds x and pass 1 holds ~x, so every bit cell is
// checked holding a 0 and holding a 1.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define CRO_PATTERN_HD __host__ __device__
#else
#define CRO_PATTERN_HD
#endif

CRO_PATTERN_HD static inline uint32_t cro_pattern_mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// invert: 0 = pass 0 (x), non-zero = pass 1 (~x)
CRO_PATTERN_HD static inline uint32_t cro_pattern_word(uint64_t w, uint32_t seed,
                                                       uint32_t invert) {
  uint32_t x = (uint32_t)w ^ seed;
  x += (uint32_t)(w >> 32) * 0x9E3779B9u;
  x = cro_pattern_mix32(x);
  return invert ? ~x : x;
}

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

// words w .. w + 3 as the 16-byte vector the kernels store and compare
CRO_PATTERN_HD static inline uint4 cro_pattern_vec4(uint64_t w, uint32_t seed,
                                                    uint32_t invert) {
  uint4 v;
  v.x = cro_pattern_word(w + 0, seed, invert);
  v.y = cro_pattern_word(w + 1, seed, invert);
  v.z = cro_pattern_word(w + 2, seed, invert);
  v.w = cro_pattern_word(w + 3, seed, invert);
  return v;
}
#endif
