// Matrix-format probe stage: the C ABI, the per-wave record and its
// aggregation, the decode tables and packers of the five narrow operand
// formats, and the inputs and expected tiles of the seven matrix checks.
//
// One definition shared by the device kernel's host driver (formats.hip), the
// native agent (agent/croagent.cpp, which loads libcroformats.so at run time)
// and a host-only test program, so "what the GPU compares against", "what the
// host reports" and the numpy mirrors in nodeops/formats.py cannot drift
// apart.  Plain C++: a host compiler without HIP can include it.
//
// The seven checks (bit of the fail mask, name, instruction, K of the stage):
//
//   0 mfma_f16  v_mfma_f32_16x16x32_f16                              K = 64
//   1 mfma_fp8  v_mfma_f32_16x16x32_fp8_fp8, e4m3 x e4m3             K = 64
//   2 mfma_bf8  v_mfma_f32_32x32x16_bf8_bf8, e5m2 x e5m2             K = 32
//   3 mx_fp8    v_mfma_scale_f32_16x16x128_f8f6f4, A e4m3 (cbsz 0),
//               B e5m2 (blgp 1), scale bytes 1 and 2                 K = 256
//   4 mx_fp6    v_mfma_scale_f32_32x32x64_f8f6f4, A e2m3 (cbsz 2),
//               B e3m2 (blgp 3), scale bytes 0 and 0                 K = 128
//   5 mx_fp4    v_mfma_scale_f32_16x16x128_f8f6f4, e2m1 both (4, 4),
//               scale bytes 3 and 1                                  K = 256
//   6 mfma_f64  v_mfma_f64_16x16x4_f64                               K = 64
//
// Logical semantics of every check, whatever the lane maps are:
//
//   D[r][c] = sum_g 2^(sa[r][g]-127) 2^(sb[c][g]-127) sum_{k in block g} A[r][k] B[c][k]
//
// with 32-element K blocks g and, for the checks without scales, all scale
// factors 1.
//
// Operand storage.  Both operands are K-contiguous: A is M x K, B is N x K
// (M = N = 16 or 32).  Elements are packed little-endian along K: f16 two
// bytes, fp8 one byte, fp6 four per three bytes (element j of a row occupies
// bits 6j .. 6j+5 of the row's bit string, bit i of the string being bit i&7
// of byte i>>3), fp4 two per byte with the low nibble first, f64 eight bytes.
// Scales are one E8M0 byte per (row or column, 32-element K block), value
// 2^(e-127).
//
// Lane, packing and scale maps, lane l of 64, as proved bit-exactly on an
// MI355X through cro_formats_tile (tests/test_probe_formats_gpu.py: random
// asymmetric data, one-hot sweeps over every k of one instruction, one scale
// byte changed at a time, every op_sel):
//
//   f16 16x16x32      A[l&15][k = 8(l>>4) + j], B[l&15][same k]: half j of
//                     the lane's 4 registers, j = 0..7
//   fp8 16x16x32      A[l&15][k = 8(l>>4) + j], B likewise: byte j of the
//                     lane's 64-bit operand, j = 0..7
//   bf8 32x32x16      A[l&31][k = 8(l>>5) + j], B likewise
//   scaled 16x16x128  fp6 and fp4: lane l holds the 32 contiguous k of block
//                     l>>4 for row (A) or column (B) l&15: fp6 bits 6j..6j+5
//                     of registers 0..5, fp4 nibble j of registers 0..3 (low
//                     nibble first); the unused high registers are ignored.
//                     fp8 and bf8: NOT contiguous.  Byte j of registers 0..3
//                     is k = 16(l>>4) + j and byte j of registers 4..7 is
//                     k = 64 + 16(l>>4) + j, j = 0..15, so a 32-element block
//                     lies in one register half of two lane groups.  (With
//                     the contiguous map every unscaled product still comes
//                     out right, A and B being permuted alike; only a scale
//                     that differs between blocks shows it.)
//   scaled 32x32x64   fp6 and fp4: the same with block l>>5 and row or
//                     column l&31 (8-bit operands of this shape: not proved,
//                     not used)
//   scales            byte op_sel (0..3) of the scale register of lane l
//                     applies to K block l>>4 (l>>5) of row or column l&15
//                     (l&31) wherever the block's elements sit: for fp6 and
//                     fp4 the lane's own 32, for fp8 and bf8 as above; the
//                     other three bytes are ignored
//   f64 16x16x4       A[l&15][k = l>>4], B[l&15][k = l>>4]; result register
//                     r is row (l>>4) + 4r, column l&15 (NOT the f32 map)
//   results           16x16 f32: register r is row 4(l>>4) + r, column l&15;
//                     32x32 f32: row (r&3) + 8(r>>2) + 4(l>>5), column l&31
//
// Exact by construction.  Nothing is assumed about how the hardware orders or
// widens these sums: for each check the values come from a fixed code set
// with a common quantum q, and for every seed sum|a b| per output element
// stays below 2^24 q_a q_b (smallest scale product), 2^53 for f64, in the
// worst case over the code set.  Every partial sum in any order is then an
// integer number of quanta below 2^24 and exact in f32.  The arithmetic is
// written next to each check's parameters below.
//
// That bound is not enough for the non-scaled fp8 / bf8 instructions.  They
// align the products of one instruction to the largest and drop low bits
// (measured on an MI355X, profiles/formats_probe_mi355x.md): sums whose
// products span 14 bits, from the leading bit of the largest product to the
// quantum of the smallest, came out exact, sums spanning 16 bits did not,
// although they stayed far below 2^24 quanta.  The code sets of mfma_fp8 and
// mfma_bf8 therefore span 12 bits.  The f16 path and the
// scaled path summed every 16-bit span they were given exactly; the stage
// uses nothing wider there.
//
// Out of scope: NaN, infinity and the 0xFF scale, the sparse (smfmac)
// instructions, and rates.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "crocoverage.h"  // cro_cov_decode, cro_cov_cu_key, cro_cov_lcg

// -- operand formats ------------------------------------------------------------
// The first five numbers are the instruction's cbsz / blgp format codes.

enum {
  CRO_FMT_E4M3 = 0,  // OCP e4m3fn: bias 7, no infinity, 0x7F / 0xFF NaN
  CRO_FMT_E5M2 = 1,  // OCP e5m2: bias 15, IEEE specials
  CRO_FMT_E2M3 = 2,  // OCP fp6 e2m3: bias 1, no specials
  CRO_FMT_E3M2 = 3,  // OCP fp6 e3m2: bias 3, no specials
  CRO_FMT_E2M1 = 4,  // OCP fp4 e2m1: bias 1, no specials
  CRO_FMT_F16 = 5,   // IEEE half
  CRO_FMT_F64 = 6,   // IEEE double (never decoded from a code here)
  CRO_FMT_FORMATS = 7,
};

static inline int cro_fmt_bits(int fmt) {
  static const int bits[CRO_FMT_FORMATS] = {8, 8, 6, 6, 4, 16, 64};
  return bits[fmt];
}

// sign | ebits exponent | mbits mantissa, IEEE-like with subnormals
static inline double cro_fmt_minifloat(uint32_t code, int ebits, int mbits, int bias) {
  const uint32_t sign = (code >> (ebits + mbits)) & 1u;
  const int e = (int)((code >> mbits) & ((1u << ebits) - 1u));
  const int m = (int)(code & ((1u << mbits) - 1u));
  const double mag = e ? ldexp((double)((1 << mbits) + m), e - bias - mbits)
                       : ldexp((double)m, 1 - bias - mbits);
  return sign ? -mag : mag;
}

// The value of one code of a format (the decode tables, entry by entry).
static inline double cro_fmt_decode(int fmt, uint32_t code) {
  switch (fmt) {
    case CRO_FMT_E4M3:
      if ((code & 0x7Fu) == 0x7Fu) return NAN;
      return cro_fmt_minifloat(code & 0xFFu, 4, 3, 7);
    case CRO_FMT_E5M2:
      if (((code >> 2) & 0x1Fu) == 0x1Fu)
        return (code & 3u) ? NAN : ((code & 0x80u) ? -INFINITY : INFINITY);
      return cro_fmt_minifloat(code & 0xFFu, 5, 2, 15);
    case CRO_FMT_E2M3:
      return cro_fmt_minifloat(code & 0x3Fu, 2, 3, 1);
    case CRO_FMT_E3M2:
      return cro_fmt_minifloat(code & 0x3Fu, 3, 2, 3);
    case CRO_FMT_E2M1:
      return cro_fmt_minifloat(code & 0xFu, 2, 1, 1);
    case CRO_FMT_F16:
      if (((code >> 10) & 0x1Fu) == 0x1Fu)
        return (code & 0x3FFu) ? NAN : ((code & 0x8000u) ? -INFINITY : INFINITY);
      return cro_fmt_minifloat(code & 0xFFFFu, 5, 10, 15);
    default:
      return NAN;
  }
}

// All codes of a narrow format (256, 64 or 16 entries).
static inline int cro_fmt_table(int fmt, float* out) {
  const int n = 1 << cro_fmt_bits(fmt);
  for (int c = 0; c < n; ++c) out[c] = (float)cro_fmt_decode(fmt, (uint32_t)c);
  return n;
}

// E8M0 scale: 2^(e-127); 0xFF is NaN (out of scope)
static inline double cro_fmt_scale(uint32_t e) {
  return (e & 0xFFu) == 0xFFu ? NAN : ldexp(1.0, (int)(e & 0xFFu) - 127);
}

// f16 bits of m / 16, |m| <= 255: a normal half (2^-4 <= |v| < 16), exact
static inline uint16_t cro_fmt_f16_of_sixteenths(int m) {
  if (m == 0) return 0;
  const uint32_t sign = m < 0 ? 0x8000u : 0u;
  uint32_t mag = (uint32_t)(m < 0 ? -m : m);  // 1..255
  int top = 7;
  while (!(mag >> top)) --top;  // value = mag 2^-4, leading bit 2^(top-4)
  const uint32_t frac = (mag << (10 - top)) & 0x3FFu;
  return (uint16_t)(sign | ((uint32_t)(top - 4 + 15) << 10) | frac);
}

// -- packers --------------------------------------------------------------------

// bytes of one K-contiguous row of K elements
static inline size_t cro_fmt_row_bytes(int fmt, int K) {
  return (size_t)K * (size_t)cro_fmt_bits(fmt) / 8;
}

// n codes of 4, 6, 8 or 16 bits, little-endian along the bit string (see the
// head of the file); out holds n * bits / 8 bytes, n * bits a multiple of 8
static inline void cro_fmt_pack(int fmt, const uint16_t* codes, size_t n, uint8_t* out) {
  const int bits = cro_fmt_bits(fmt);
  memset(out, 0, n * (size_t)bits / 8);
  for (size_t i = 0; i < n; ++i)
    for (int b = 0; b < bits; ++b)
      if ((codes[i] >> b) & 1u) {
        const size_t pos = i * (size_t)bits + (size_t)b;
        out[pos >> 3] |= (uint8_t)(1u << (pos & 7));
      }
}

static inline void cro_fmt_unpack(int fmt, const uint8_t* in, size_t n, uint16_t* codes) {
  const int bits = cro_fmt_bits(fmt);
  for (size_t i = 0; i < n; ++i) {
    uint32_t c = 0;
    for (int b = 0; b < bits; ++b) {
      const size_t pos = i * (size_t)bits + (size_t)b;
      c |= (uint32_t)((in[pos >> 3] >> (pos & 7)) & 1u) << b;
    }
    codes[i] = (uint16_t)c;
  }
}

// -- the seven checks -------------------------------------------------------------

enum {
  CRO_FMT_TEST_F16 = 0,
  CRO_FMT_TEST_FP8 = 1,
  CRO_FMT_TEST_BF8 = 2,
  CRO_FMT_TEST_MX_FP8 = 3,
  CRO_FMT_TEST_MX_FP6 = 4,
  CRO_FMT_TEST_MX_FP4 = 5,
  CRO_FMT_TEST_F64 = 6,
  CRO_FMT_TESTS = 7,
};

// The stage's scale byte selects (op_sel): immediates of the instruction, so
// named here for the kernel; two of the three checks use non-zero ones.
enum {
  CRO_FMT_MX_FP8_SEL_A = 1,
  CRO_FMT_MX_FP8_SEL_B = 2,
  CRO_FMT_MX_FP6_SEL_A = 0,
  CRO_FMT_MX_FP6_SEL_B = 0,
  CRO_FMT_MX_FP4_SEL_A = 3,
  CRO_FMT_MX_FP4_SEL_B = 1,
};

enum {
  CRO_FMT_MAX_ELEMS = 32 * 32,     // largest result tile
  CRO_FMT_MAX_OPERAND = 16 * 256,  // largest M * K of the stage (= 32 * 128)
  CRO_FMT_MAX_PACKED = 16 * 64 * 8,  // largest packed operand of the stage (f64)
  CRO_FMT_MAX_SCALES = 16 * 8,     // largest M * K / 32 (= 32 * 4)
  CRO_FMT_MAX_TILE_K = 4096,       // cro_formats_tile: largest K
};

// Code sets: a code is sign | exponent field | mantissa with the exponent
// field drawn from e_lo .. e_lo + e_n - 1 and every mantissa and both signs.
// q is the common quantum of the set, max its largest magnitude in quanta.
struct CroFmtTestDesc {
  const char* name;
  int m;      // rows of A = rows of B = M = N
  int k;      // K of the stage
  int kstep;  // K of one instruction
  int fmt_a, e_lo_a, e_n_a;
  int fmt_b, e_lo_b, e_n_b;
  int scale_base_a, scale_base_b, scale_spread;  // bytes base-spread .. base+spread; 0 0 0: none
  int op_sel_a, op_sel_b;                        // the stage's scale byte selects
  uint32_t lcg_salt;
};

static inline const CroFmtTestDesc* cro_fmt_test(int test) {
  static const CroFmtTestDesc tests[CRO_FMT_TESTS] = {
      // m / 16, |m| <= 255: q = 2^-4 both sides, max 255 q.
      // 255 * 255 * 64 = 4 161 600 < 2^24 = 16 777 216 quanta q^2.
      {"mfma_f16", 16, 64, 32, CRO_FMT_F16, 0, 0, CRO_FMT_F16, 0, 0, 0, 0, 0, 0, 0, 0x27d4eb2fu},
      // e4m3 fields 7..9: (8 + m) 2^(e-10), q = 2^-3 (e = 7), max 7.5 = 60 q (e = 9).
      // 60 * 60 * 64 = 230 400 < 2^24.  Span: the largest product 3600 q^2
      // has its leading bit at 2^11, the smallest quantum is q^2: 12 bits.
      {"mfma_fp8", 16, 64, 32, CRO_FMT_E4M3, 7, 3, CRO_FMT_E4M3, 7, 3, 0, 0, 0, 0, 0,
       0x165667b1u},
      // e5m2 fields 14..17: (4 + m) 2^(e-17), q = 2^-3 (e = 14), max 7 = 56 q (e = 17).
      // 56 * 56 * 32 = 100 352 < 2^24.  Span: 3136 q^2, leading bit 2^11: 12 bits.
      {"mfma_bf8", 32, 32, 16, CRO_FMT_E5M2, 14, 4, CRO_FMT_E5M2, 14, 4, 0, 0, 0, 0, 0,
       0xd3a2646cu},
      // A e4m3 fields 7..9: q = 2^-3, max 7.5 = 60 q.  B e5m2 fields 15..17:
      // q = 2^-2, max 7 = 28 q.  Scale bytes base-1..base+1 per side: a scale
      // product is 1, 2, 4, 8 or 16 times the smallest.
      // 60 * 28 * 16 * 256 = 6 881 280 < 2^24.
      {"mx_fp8", 16, 256, 128, CRO_FMT_E4M3, 7, 3, CRO_FMT_E5M2, 15, 3, 120, 134, 1,
       CRO_FMT_MX_FP8_SEL_A, CRO_FMT_MX_FP8_SEL_B, 0xfd7046c5u},
      // A all e2m3 codes: q = 2^-3, max 7.5 = 60 q.  B e3m2 fields 2..5:
      // (4 + m) 2^(e-5), q = 2^-3 (e = 2), max 7 = 56 q (e = 5).  Scales as above.
      // 60 * 56 * 16 * 128 = 6 881 280 < 2^24.
      {"mx_fp6", 32, 128, 64, CRO_FMT_E2M3, 0, 4, CRO_FMT_E3M2, 2, 4, 120, 134, 1,
       CRO_FMT_MX_FP6_SEL_A, CRO_FMT_MX_FP6_SEL_B, 0xb55a4f09u},
      // all 16 e2m1 codes both sides: q = 2^-1, max 6 = 12 q.  Scale bytes
      // base-2..base+2 per side: a scale product is up to 2^8 times the smallest.
      // 12 * 12 * 256 * 256 = 9 437 184 < 2^24.
      {"mx_fp4", 16, 256, 128, CRO_FMT_E2M1, 0, 4, CRO_FMT_E2M1, 0, 4, 120, 134, 2,
       CRO_FMT_MX_FP4_SEL_A, CRO_FMT_MX_FP4_SEL_B, 0x2545f491u},
      // integers of magnitude below 2^20, q = 1: 2^20 * 2^20 * 64 = 2^46 < 2^53.
      {"mfma_f64", 16, 64, 4, CRO_FMT_F64, 0, 0, CRO_FMT_F64, 0, 0, 0, 0, 0, 0, 0, 0x9e3779b1u},
  };
  return &tests[test];
}

// K of the stage as a constant expression (the kernel's loop bounds); the
// same numbers as the table's
static constexpr int cro_fmt_k(int test) {
  return test == CRO_FMT_TEST_MX_FP8 || test == CRO_FMT_TEST_MX_FP4 ? 256
         : test == CRO_FMT_TEST_MX_FP6                              ? 128
         : test == CRO_FMT_TEST_BF8                                 ? 32
                                                                    : 64;
}

static inline int cro_fmt_elems(int test) {
  const int m = cro_fmt_test(test)->m;
  return m * m;
}

// lowest failing check of a fail mask
static inline const char* cro_fmt_test_name(uint32_t fail_mask) {
  for (int t = 0; t < CRO_FMT_TESTS; ++t)
    if (fail_mask & (1u << t)) return cro_fmt_test(t)->name;
  return "";
}

// -- inputs -------------------------------------------------------------------------

// One check's inputs: the codes and the values they decode to, element
// [row][k] at row * K + k, the packed operands as the device reads them, and
// the scale bytes [row][block] (all 127, factor 1, where the check has none).
struct CroFmtInputs {
  int test;
  uint16_t codes_a[CRO_FMT_MAX_OPERAND], codes_b[CRO_FMT_MAX_OPERAND];
  double val_a[CRO_FMT_MAX_OPERAND], val_b[CRO_FMT_MAX_OPERAND];
  uint8_t scale_a[CRO_FMT_MAX_SCALES], scale_b[CRO_FMT_MAX_SCALES];
  // 8-byte aligned: the f64 operands live here as doubles
  alignas(8) uint8_t packed_a[CRO_FMT_MAX_PACKED];
  alignas(8) uint8_t packed_b[CRO_FMT_MAX_PACKED];
};

// One draw of the LCG to one code of a set: sign bit 31, mantissa bits 30..28
// (the low mbits of them), exponent field e_lo + (bits 23..8) mod e_n.
static inline uint16_t cro_fmt_draw_code(uint32_t x, int fmt, int e_lo, int e_n) {
  static const int ebits[5] = {4, 5, 2, 3, 2}, mbits[5] = {3, 2, 3, 2, 1};
  const uint32_t sign = x >> 31;
  const uint32_t mant = (x >> 28) & ((1u << mbits[fmt]) - 1u);
  const uint32_t e = (uint32_t)e_lo + ((x >> 8) & 0xFFFFu) % (uint32_t)e_n;
  return (uint16_t)((sign << (ebits[fmt] + mbits[fmt])) | (e << mbits[fmt]) | mant);
}

static inline void cro_fmt_draw_operand(uint32_t* s, int test, int fmt, int e_lo, int e_n, int n,
                                        uint16_t* codes, double* vals, uint8_t* packed) {
  for (int i = 0; i < n; ++i) {
    const uint32_t x = cro_cov_lcg(s);
    if (test == CRO_FMT_TEST_F16) {
      const int mag = (int)((x >> 8) & 0xFFu);
      const int m = (x >> 31) ? -mag : mag;
      codes[i] = cro_fmt_f16_of_sixteenths(m);
      vals[i] = (double)m / 16.0;
    } else if (test == CRO_FMT_TEST_F64) {
      const int mag = (int)((x >> 8) & 0xFFFFFu);
      codes[i] = 0;
      vals[i] = (x >> 31) ? -(double)mag : (double)mag;
    } else {
      codes[i] = cro_fmt_draw_code(x, fmt, e_lo, e_n);
      vals[i] = cro_fmt_decode(fmt, codes[i]);
    }
  }
  if (test == CRO_FMT_TEST_F64)
    memcpy(packed, vals, (size_t)n * sizeof(double));
  else
    cro_fmt_pack(fmt, codes, (size_t)n, packed);
}

// A, then B, then A's scales, then B's, from one LCG stream per check and seed.
static inline void cro_fmt_make(int test, uint32_t seed, CroFmtInputs* in) {
  const CroFmtTestDesc* d = cro_fmt_test(test);
  uint32_t s = d->lcg_salt ^ seed;
  const int n = d->m * d->k, ns = d->m * (d->k / 32);
  memset(in, 0, sizeof(*in));
  in->test = test;
  cro_fmt_draw_operand(&s, test, d->fmt_a, d->e_lo_a, d->e_n_a, n, in->codes_a, in->val_a,
                       in->packed_a);
  cro_fmt_draw_operand(&s, test, d->fmt_b, d->e_lo_b, d->e_n_b, n, in->codes_b, in->val_b,
                       in->packed_b);
  const uint32_t width = 2u * (uint32_t)d->scale_spread + 1u;
  for (int i = 0; i < ns; ++i)
    in->scale_a[i] = d->scale_base_a
                         ? (uint8_t)(d->scale_base_a - d->scale_spread +
                                     (int)((cro_cov_lcg(&s) >> 24) % width))
                         : 127;
  for (int i = 0; i < ns; ++i)
    in->scale_b[i] = d->scale_base_b
                         ? (uint8_t)(d->scale_base_b - d->scale_spread +
                                     (int)((cro_cov_lcg(&s) >> 24) % width))
                         : 127;
}

// The logical product of the head of the file, in double: every term and
// every partial sum is exact there (the bounds above leave 29 bits to spare),
// so the order of summation does not matter.  A M x K, B M x K, scales
// M x K/32, D M x M; K a multiple of 32.
static inline void cro_fmt_product(const double* A, const double* B, const uint8_t* sa,
                                   const uint8_t* sb, int M, int K, double* D) {
  const int G = K / 32;
  for (int r = 0; r < M; ++r)
    for (int c = 0; c < M; ++c) {
      double acc = 0.0;
      for (int g = 0; g < G; ++g) {
        double part = 0.0;
        for (int k = 32 * g; k < 32 * g + 32; ++k) part += A[r * K + k] * B[c * K + k];
        acc += cro_fmt_scale(sa[r * G + g]) * cro_fmt_scale(sb[c * G + g]) * part;
      }
      D[r * M + c] = acc;
    }
}

// The expected tile as the device compares it: float bits for checks 0..5
// (one word per element), double bits for mfma_f64 (two words per element,
// low word first).  Returns the number of 32-bit words.
static inline int cro_fmt_expected(const CroFmtInputs* in, uint32_t* words) {
  const CroFmtTestDesc* d = cro_fmt_test(in->test);
  double D[CRO_FMT_MAX_ELEMS];
  cro_fmt_product(in->val_a, in->val_b, in->scale_a, in->scale_b, d->m, d->k, D);
  const int elems = d->m * d->m;
  if (in->test == CRO_FMT_TEST_F64) {
    memcpy(words, D, (size_t)elems * sizeof(double));
    return 2 * elems;
  }
  for (int i = 0; i < elems; ++i) {
    const float f = (float)D[i];
    memcpy(&words[i], &f, sizeof(f));
  }
  return elems;
}

// Largest sum over k of |a b| (scale product) of any output element, in
// quanta q_a q_b (smallest scale product of the check): what has to stay
// below 2^24 (2^53 for f64).
static inline double cro_fmt_abs_quanta(const CroFmtInputs* in) {
  static const double q[CRO_FMT_TESTS][2] = {
      {0.0625, 0.0625}, {0.125, 0.125}, {0.125, 0.125}, {0.125, 0.25},
      {0.125, 0.125},   {0.5, 0.5},       {1.0, 1.0}};
  const CroFmtTestDesc* d = cro_fmt_test(in->test);
  const int M = d->m, K = d->k, G = K / 32;
  const double smin = d->scale_base_a
                          ? cro_fmt_scale((uint32_t)(d->scale_base_a - d->scale_spread)) *
                                cro_fmt_scale((uint32_t)(d->scale_base_b - d->scale_spread))
                          : 1.0;
  double worst = 0.0;
  for (int r = 0; r < M; ++r)
    for (int c = 0; c < M; ++c) {
      double acc = 0.0;
      for (int k = 0; k < K; ++k)
        acc += fabs(in->val_a[r * K + k] * in->val_b[c * K + k]) *
               cro_fmt_scale(in->scale_a[r * G + k / 32]) *
               cro_fmt_scale(in->scale_b[c * G + k / 32]);
      if (acc > worst) worst = acc;
    }
  return worst / (q[in->test][0] * q[in->test][1] * smin);
}

// -- record and aggregation -----------------------------------------------------

// One per wave and round, written by lane 0.  n_bad sums over the failing
// checks; first_bad and bits_bad belong to the failing check with the lowest
// mask bit (the one cro_fmt_test_name names): the element index row * M + col
// and the OR of got ^ want (for mfma_f64 of both 32-bit halves).
struct CroFormatsRecord {
  uint32_t xcc_id;     // raw XCC_ID register
  uint32_t hw_id;      // raw HW_ID register
  uint32_t fail_mask;  // bit t: check t
  uint32_t n_bad;      // values that differed
  uint32_t first_bad;  // lowest bad element; ~0 = none
  uint32_t bits_bad;
  uint32_t valid;  // 1 once a wave wrote the record
  uint32_t reserved;
};

struct CroFormatsAgg {
  unsigned long long waves_run;            // valid records
  unsigned long long waves_bad;            // records with a non-zero fail mask
  unsigned long long bad[CRO_FMT_TESTS];   // bad waves per check, from the fail mask
  long long first_bad_index;               // index of the first bad record; -1 = none
  int cus_seen;                            // distinct CU keys
  int xcds_seen;
  int simds_seen;  // distinct (CU key, SIMD) pairs
  int cus_bad;     // distinct CU keys with a bad wave
  // the first bad wave (lowest record index); -1 / 0 when there is none
  int xcd, se, sh, cu, simd;
  unsigned int first_fail_mask;
  unsigned int n_bad;
  unsigned int first_bad;
  unsigned int bits_bad;
  unsigned int reserved;  // to a multiple of 8 bytes: the flat mirrors have no hole
};

// cro_wave_summarize (crocoverage.h); over no records the cleared aggregate.
static inline void cro_formats_aggregate(const CroFormatsRecord* records, size_t n,
                                         CroFormatsAgg* out) {
  CroWaveSummary s;
  cro_wave_summarize(records, n, &s);
  cro_wave_common(s, out);
  for (int t = 0; t < CRO_FMT_TESTS; ++t) out->bad[t] = s.bad[t];
}

// -- C ABI (libcroformats.so) -----------------------------------------------------

// Zero takes the library default.  The selftest_* options are for tests:
// wrong data, in bounds.
//   mode 1  the host flips bit selftest_bit of element selftest_elem of the
//           EXPECTED tile of check selftest_test: every wave must flag it
//           (with selftest_also = 1 + t2, the host flips the same bit of
//           element selftest_elem + 1 of check t2's expected tile as well:
//           two checks fail in one wave)
//   mode 2  the kernel flips that bit of its COMPUTED value on the waves whose
//           CU key (cro_cov_cu_key) is selftest_key: exactly those flag it
// selftest_bit is 0..31, for mfma_f64 0..63.
struct CroFormatsOpts {
  int grid_blocks;  // workgroups; default one per CU
  int iters;        // repeats of the seven products per wave
  int max_rounds;   // bounded relaunch while a CU or SIMD is unseen
  unsigned int seed;
  int selftest_mode;
  int selftest_test;
  int selftest_bit;
  unsigned int selftest_elem;
  unsigned int selftest_key;
  int selftest_also;
  double min_cu_fraction;  // > 0: fewer CUs seen than this fraction is rc -33
};

struct CroFormatsResult {
  int ok;
  int rc;  // 0 ok, -1 HIP error or bad argument, -32 format mismatch, -33 CU-coverage floor
  int cus_expected;
  int rounds;
  struct CroFormatsAgg agg;
  int first_bad_round;
  int first_bad_record;
  int grid_blocks;
  int iters;
  double gpu_ms;
  double t_total_ms;
  char failed_test[16];
  char msg[256];
};

#ifdef __cplusplus
extern "C" {
#endif

int cro_formats_run(int device, const struct CroFormatsOpts* opts, struct CroFormatsResult* out);

// cro_formats_run, and the rounds' raw records (at most max_records), round-major.
int cro_formats_run_records(int device, const struct CroFormatsOpts* opts,
                            struct CroFormatsResult* out, struct CroFormatsRecord* records_out,
                            int max_records);

// One wave of the stage's own product code on caller data (for tests): A and
// B packed M x K as above, scales M x K/32 (ignored, may be null, for the
// checks without scales), D M x M float (double for mfma_f64).  K a multiple
// of the instruction's K, at most 4096; op_sel_a / op_sel_b 0..3 (0 for the
// checks without scales).  0 ok, -10 bad argument, -1 HIP error.
int cro_formats_tile(int device, int test, int op_sel_a, int op_sel_b, const void* A,
                     const void* B, const unsigned char* scale_a, const unsigned char* scale_b,
                     void* D, int K);

#ifdef __cplusplus
}
#endif
