// ALU probe stage: exact checks of the vector and scalar ALUs on every SIMD,
// with fault location.
//
// Everything the host decides lives here: the one list of FORMS (the
// instruction, its inline-asm template, its operand signature, its operand
// class and its host reference), the operand table the device reads, the
// per-wave record, the aggregation (with the transcendental consensus) and the
// C ABI of libcroalu.so.  One definition shared by the device kernel
// (alu.hip), the native agent, a host-only test program and the mirror in
// nodeops/alu.py, which states every reference a second time in numpy / pure
// Python.  Plain C++: a host compiler without HIP can include it.
//
// A form is one asm statement run on 64 ROWS of operands.  A row is eight
// words: six source words s[0..5] (operands laid out one after the other, a
// 64-bit operand low word first) and the two expected result words.  At
// repeat r lane l takes row (l + r) & 63; the scalar forms take row r & 63 in
// every lane.  The first rows of a form are the fixed edge rows of its
// operand class, the others come from the seeded LCG.
//
// Checks, in fail-mask bit order: int_arith, bit_ops, pk_int, dot, f32, f16,
// f64, convert, scale_convert, compare_select, salu, transcendental.
//
// Exactness.  Every expected word is one rounding of an exactly computed
// value, so a C++ and a Python reference agree bit for bit:
//   f32 / f16 fma   for non-zero operands -5 <= e(a) + e(b) - e(c) <= 26
//                   (e = floor(log2 |x|)): then a * b + c is exact in f64
//                   (at most 53 significant bits) and the result is one
//                   rounding of it (CRO_ALU_FMA_LO / _HI below)
//   f64 add, mul, fma  operands are 21-bit integers times a power of two,
//                   close enough that the exact result fits 53 bits
//   f64 divide, sqrt   IEEE-correct on both sides (plain a / b, sqrt)
//   float dots      integer-valued operands, sums exact in any order
// Subnormal inputs and results are kept: the kernel runs in the compiler's
// default mode (f32 and f64/f16 denormals on), which a test reads in the
// kernel descriptor.
//
// transcendental: results are not derivable on the host.  The first
// CRO_ALU_ANCHORS rows of such a form are ANCHORS (results any correct
// implementation gives exactly, compared like every other word); every result
// word of every row is folded into the wave's digest, which must be the one a
// strict majority of the waves holds.  Consensus cannot see a fault common to
// all SIMDs: only the anchors catch that.
//
// Not covered: see docs/architecture.md.
#pragma once

#include "crocoverage.h"
#include "croformats.h"

enum {
  CRO_ALU_INT = 0,
  CRO_ALU_BIT = 1,
  CRO_ALU_PKINT = 2,
  CRO_ALU_DOT = 3,
  CRO_ALU_F32 = 4,
  CRO_ALU_F16 = 5,
  CRO_ALU_F64 = 6,
  CRO_ALU_CVT = 7,
  CRO_ALU_SCALE = 8,
  CRO_ALU_CMP = 9,
  CRO_ALU_SALU = 10,
  CRO_ALU_TRANS = 11,
  CRO_ALU_TESTS = 12,
};

enum {
  CRO_ALU_ROWS = 64,
  CRO_ALU_ROW_WORDS = 8,  // s[0..5], want[0..1]
  CRO_ALU_ANCHORS = 16,   // anchor rows of a transcendental form
  CRO_ALU_FMA_LO = -5,    // bound on e(a) + e(b) - e(c) of an fma row
  CRO_ALU_FMA_HI = 26,
};

static const char* const kCroAluTestNames[CRO_ALU_TESTS] = {
    "int_arith", "bit_ops", "pk_int",        "dot",            "f32",  "f16",
    "f64",       "convert", "scale_convert", "compare_select", "salu", "transcendental"};

static inline const char* cro_alu_test_name(uint32_t fail_mask) {
  for (int t = 0; t < CRO_ALU_TESTS; ++t)
    if (fail_mask & (1u << t)) return kCroAluTestNames[t];
  return "";
}

// -- operand signatures ---------------------------------------------------------------
// X(name, source words, result words).  V: a 32-bit VGPR operand, D: a 64-bit
// VGPR pair, O: the destination's previous content (`old`, the last source
// word), S / Q: a uniform 32 / 64-bit SGPR operand.  The first letters name
// the result: V1 one VGPR, V2 a pair, S1 / S2 scalar, S1C a scalar and SCC,
// SC the SCC alone (of a form whose result fills both words: the instruction
// runs again in a statement of its own that captures SCC).  V1_MBCNT: the
// result depends on the lane; the table holds it for lane = row.  V2_FP6: one
// 192-bit operand (32 six-bit codes); the 32 result registers are folded
// into two words, rotate-left-5 and xor over the even and over the odd ones,
// by plain C++ after the statement.
#define CRO_ALU_SIGS(X)                                                                          \
  X(V1_V, 1, 1) X(V1_VV, 2, 1) X(V1_VVV, 3, 1) X(V1_VVO, 3, 1) X(V1_VVVO, 4, 1) X(V1_MBCNT, 3, 1) \
  X(V2_D, 2, 2) X(V2_DD, 4, 2) X(V2_DDD, 6, 2) X(V2_VD, 3, 2) X(V2_DV, 3, 2) X(V2_VVD, 4, 2)    \
  X(V2_V, 1, 2) X(V2_VV, 2, 2) X(V1_D, 2, 1) X(V1_DD, 4, 1) X(V1_DV, 3, 1) X(V2C_VVVV, 4, 2)    \
  X(V1_CMPX, 3, 1) X(X_DIV, 4, 2) X(X_SQRT, 2, 2) X(V2_FP6, 6, 2)                                                \
  X(S1_S, 1, 1) X(S1_SS, 2, 1) X(S1_SSSS, 4, 1) X(S1C_S, 1, 2) X(S1C_SS, 2, 2)                  \
  X(S2_Q, 2, 2) X(S2_QQ, 4, 2) X(S2_QS, 3, 2) X(S1_Q, 2, 1) X(S1C_Q, 2, 2) X(S2C_SSSS, 4, 2)       \
  X(SC_QQ, 4, 1) X(SC_QS, 3, 1) X(SC_SSSS, 4, 1)

enum {
#define CRO_ALU_X(name, nsrc, nres) CRO_ALU_SIG_##name,
  CRO_ALU_SIGS(CRO_ALU_X)
#undef CRO_ALU_X
      CRO_ALU_SIG_COUNT
};
enum {
#define CRO_ALU_X(name, nsrc, nres) CRO_ALU_NSRC_##name = nsrc, CRO_ALU_NRES_##name = nres,
  CRO_ALU_SIGS(CRO_ALU_X)
#undef CRO_ALU_X
};

// -- operand classes ------------------------------------------------------------------
enum {
  CRO_ALU_C_INT,     // integer words: edge rows kCroAluIntEdges
  CRO_ALU_C_PERM,    // as INT; the selector bytes of s2 are 0..15, the first rows hold all 16
  CRO_ALU_C_F32,     // f32 in every word
  CRO_ALU_C_F32FMA,  // (s0, s1, s2) and (s3, s4, s5) within the fma bound
  CRO_ALU_C_F32PKFMA,  // (s0, s2, s4) and (s1, s3, s5) within the fma bound
  CRO_ALU_C_F32I,    // s0 f32, s1 a small integer (ldexp)
  CRO_ALU_C_F32U8,   // s0 f32 around 0..256 with ties, s1 a byte select, s2 old
  CRO_ALU_C_F32NORM, // s0, s1 f32 around -1..1 with the clamps
  CRO_ALU_C_SCALEF16,  // s0 two halves, s1 the scale, s2 old
  CRO_ALU_C_SCALEBF16,
  CRO_ALU_C_F32CVT,  // f32 around the integer range, with NaN and infinities
  CRO_ALU_C_F32H,    // f32 in and around the f16 range, with ties
  CRO_ALU_C_F16,     // two halves in every word
  CRO_ALU_C_F16FMA,  // halves of (s0, s1, s2) within the fma bound, low and high
  CRO_ALU_C_F64,     // 21-bit integers times 2^e, as s0:s1, s2:s3, s4:s5
  CRO_ALU_C_F64FMA,  // the same, c placed so that a * b + c fits 53 bits
  CRO_ALU_C_F64R,    // full-mantissa doubles (rounding ops, divide, sqrt, converts)
  CRO_ALU_C_F64DIV,  // as F64R without the zero row, s0:s1 not negative (divide, sqrt)
  CRO_ALU_C_F64I,    // s0:s1 f64, s2 a small integer
  CRO_ALU_C_DOTF16,  // integer-valued halves, s2 an integer-valued f32
  CRO_ALU_C_DOTBF16,
  CRO_ALU_C_FP8,     // s0 fp8 codes, s1 a power-of-two f32 scale
  CRO_ALU_C_BF8,
  CRO_ALU_C_FP4,
  CRO_ALU_C_FP6,     // six words of 6-bit codes (every code is a number)
  CRO_ALU_C_SCALEF32,  // s0, s1 f32, s2 the scale, s3 old
  CRO_ALU_C_CMPF32,  // pairs from a pool with NaN, +-0, equal values
  CRO_ALU_C_CMPF64,  // pool without NaN
  CRO_ALU_C_CMPF16,
  CRO_ALU_C_CMPINT,  // integer pairs, often equal
  CRO_ALU_C_CLASS32,  // s0 a value of each class, s1 the class mask
  CRO_ALU_C_CLASS64,
  CRO_ALU_C_TEXP, CRO_ALU_C_TLOG, CRO_ALU_C_TRCP, CRO_ALU_C_TSQRT, CRO_ALU_C_TSIN,
  CRO_ALU_C_TRCP64, CRO_ALU_C_TSQRT64,
  CRO_ALU_C_TEXP16, CRO_ALU_C_TLOG16, CRO_ALU_C_TRCP16, CRO_ALU_C_TSQRT16,
};

// -- bit casts and roundings -----------------------------------------------------------

static inline float cro_alu_f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t cro_alu_u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline double cro_alu_d(uint32_t lo, uint32_t hi) {
  const uint64_t u = ((uint64_t)hi << 32) | lo; double d; memcpy(&d, &u, 8); return d;
}
static inline uint64_t cro_alu_ud(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
static inline void cro_alu_w64(uint32_t* w, uint64_t v) { w[0] = (uint32_t)v; w[1] = (uint32_t)(v >> 32); }
static inline void cro_alu_wd(uint32_t* w, double d) { cro_alu_w64(w, cro_alu_ud(d)); }
static inline int cro_alu_ilogb(double x) { int e; frexp(x, &e); return e - 1; }

static inline double cro_alu_h(uint32_t code) { return cro_fmt_decode(CRO_FMT_F16, code & 0xFFFFu); }

// one rounding of a double to a half: mode 0 nearest-even, 1 toward zero
static inline uint32_t cro_alu_h_of(double x, int rtz = 0) {
  const uint32_t sign = signbit(x) ? 0x8000u : 0u;
  double a = fabs(x);
  if (a != a) return 0x7E00u;
  if (a == 0.0) return sign;
  if (isinf(a)) return sign | 0x7C00u;
  int q = cro_alu_ilogb(a) - 10;
  if (q < -24) q = -24;
  const double scaled = ldexp(a, -q);  // exact
  const double n = rtz ? floor(scaled) : nearbyint(scaled);
  double r = ldexp(n, q);
  if (r > 65504.0) {
    if (rtz) r = 65504.0; else return sign | 0x7C00u;
  }
  if (r == 0.0) return sign;
  const int e = cro_alu_ilogb(r);
  if (e < -14) return sign | (uint32_t)ldexp(r, 24);
  return sign | ((uint32_t)(e + 15) << 10) | ((uint32_t)ldexp(r, 10 - e) & 0x3FFu);
}

static inline uint32_t cro_alu_bf16_of(uint32_t u) {  // nearest-even, of finite f32 bits
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

static inline uint32_t cro_alu_lcg(uint32_t s) { return s * 1664525u + 1013904223u; }

// word k of row `row` of form `form`
static inline uint32_t cro_alu_rand(uint32_t seed, int form, int row, int k) {
  uint32_t x = seed ^ 0xA10C0DEu ^ ((uint32_t)((form * 64 + row) * 8 + k) * 0x9E3779B9u);
  x = cro_alu_lcg(cro_alu_lcg(x));
  x ^= x >> 15;
  x = cro_alu_lcg(x);
  return x ^ (x >> 13);
}

static inline int32_t cro_alu_sx(uint32_t v, int bits) {
  const uint32_t m = 1u << (bits - 1);
  v &= (m << 1) - 1u;
  return (int32_t)((v ^ m) - m);
}
static inline uint32_t cro_alu_clz(uint32_t v) { uint32_t n = 0; while (n < 32 && !(v & (0x80000000u >> n))) ++n; return n; }
static inline uint32_t cro_alu_ctz(uint32_t v) { uint32_t n = 0; while (n < 32 && !(v & (1u << n))) ++n; return n; }
CRO_COV_HD static inline uint32_t cro_alu_pop(uint64_t v) { uint32_t n = 0; for (; v; v &= v - 1) ++n; return n; }
static inline uint32_t cro_alu_rev(uint32_t v) { uint32_t r = 0; for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i); return r; }
static inline int64_t cro_alu_sat(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// -- references ------------------------------------------------------------------------
// void ref(const uint32_t* s, uint32_t* w).  Inside: a..f are s[0..5]; A, B, C
// the 64-bit operands s1:s0, s3:s2, s5:s4; fa.. the f32 and da.. the f64 views.

#define CRO_ALU_REF_HEAD                                                                        \
  const uint32_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5];                    \
  const uint64_t A = ((uint64_t)b << 32) | a, B = ((uint64_t)d << 32) | c,                      \
                 C = ((uint64_t)f << 32) | e;                                                   \
  const float fa = cro_alu_f(a), fb = cro_alu_f(b), fc = cro_alu_f(c);                          \
  const double da = cro_alu_d(a, b), db = cro_alu_d(c, d), dc = cro_alu_d(e, f);                \
  (void)a; (void)b; (void)c; (void)d; (void)e; (void)f; (void)A; (void)B; (void)C; (void)fa;    \
  (void)fb; (void)fc; (void)da; (void)db; (void)dc; w[0] = w[1] = 0;

#define R1(name, expr) static inline void cro_alu_r_##name(const uint32_t* s, uint32_t* w) { CRO_ALU_REF_HEAD w[0] = (uint32_t)(expr); }
#define R2(name, expr) static inline void cro_alu_r_##name(const uint32_t* s, uint32_t* w) { CRO_ALU_REF_HEAD cro_alu_w64(w, (uint64_t)(expr)); }
#define RF(name, expr) static inline void cro_alu_r_##name(const uint32_t* s, uint32_t* w) { CRO_ALU_REF_HEAD w[0] = cro_alu_u((float)(expr)); }
#define RD(name, expr) static inline void cro_alu_r_##name(const uint32_t* s, uint32_t* w) { CRO_ALU_REF_HEAD cro_alu_wd(w, (double)(expr)); }
#define RB(name, ...) static inline void cro_alu_r_##name(const uint32_t* s, uint32_t* w) { CRO_ALU_REF_HEAD __VA_ARGS__ }
// per 16-bit half: x, y, z the halves of a, b, c
#define RH(name, expr) static inline void cro_alu_r_##name(const uint32_t* s, uint32_t* w) { CRO_ALU_REF_HEAD \
  for (int h = 0; h < 2; ++h) { const uint32_t x = (a >> (16 * h)) & 0xFFFFu, y = (b >> (16 * h)) & 0xFFFFu, z = (c >> (16 * h)) & 0xFFFFu; \
    (void)x; (void)y; (void)z; w[0] |= ((uint32_t)(expr) & 0xFFFFu) << (16 * h); } }
#define SX16(v) cro_alu_sx(v, 16)
#define HF(v) cro_alu_h(v)

// int_arith
R2(add_u64, A + B)
R2(sub_u64, A - B)
R1(mul_lo_u32, a * b)
R1(mul_hi_u32, ((uint64_t)a * b) >> 32)
R1(mul_hi_i32, (uint64_t)((int64_t)(int32_t)a * (int32_t)b) >> 32)
R2(mad_u64_u32, (uint64_t)a * b + (((uint64_t)d << 32) | c))
R2(mad_i64_i32, (uint64_t)((int64_t)(int32_t)a * (int32_t)b) + (((uint64_t)d << 32) | c))
R1(mad_u32_u24, (a & 0xFFFFFFu) * (b & 0xFFFFFFu) + c)
R1(mul_i32_i24, (uint32_t)cro_alu_sx(a, 24) * (uint32_t)cro_alu_sx(b, 24))
R1(lshl_add_u32, (a << (b & 31u)) + c)
R1(add3_u32, a + b + c)
RB(sad_u8, uint32_t r = c; for (int i = 0; i < 4; ++i) { const int x = (a >> (8 * i)) & 255, y = (b >> (8 * i)) & 255; r += (uint32_t)(x > y ? x - y : y - x); } w[0] = r;)
// bit_ops (the ..rev shifts take the count first; the 64-bit value is s2:s1)
R1(lshlrev_b32, b << (a & 31u))
R1(lshrrev_b32, b >> (a & 31u))
R1(ashrrev_i32, (uint32_t)((int32_t)b >> (a & 31u)))
R2(lshlrev_b64, (((uint64_t)c << 32) | b) << (a & 63u))
R2(lshrrev_b64, (((uint64_t)c << 32) | b) >> (a & 63u))
R2(ashrrev_i64, (uint64_t)((int64_t)(((uint64_t)c << 32) | b) >> (a & 63u)))
RB(bfe_u32, const uint32_t o = b & 31u, n = c & 31u; w[0] = n ? (a >> o) & ((1u << n) - 1u) : 0u;)
RB(bfe_i32, const uint32_t o = b & 31u, n = c & 31u;
   w[0] = !n ? 0u : o + n < 32 ? (uint32_t)((int32_t)(a << (32 - o - n)) >> (32 - n)) : (uint32_t)((int32_t)a >> o);)
R1(bfi_b32, (a & b) | (~a & c))
R1(alignbit_b32, ((((uint64_t)a << 32) | b) >> (c & 31u)))
R1(alignbyte_b32, ((((uint64_t)a << 32) | b) >> (8u * (c & 3u))))
RB(perm_b32, const uint64_t in = ((uint64_t)a << 32) | b; uint32_t r = 0;
   for (int i = 0; i < 4; ++i) { const uint32_t sel = (c >> (8 * i)) & 255u; uint32_t v;
     if (sel >= 13) v = 0xFF; else if (sel == 12) v = 0; else if (sel >= 8) v = ((in >> (16 * (sel - 8) + 15)) & 1u) ? 0xFF : 0;
     else v = (uint32_t)(in >> (8 * sel)) & 255u; r |= v << (8 * i); } w[0] = r;)
static inline uint32_t cro_alu_bitop3(uint32_t a, uint32_t b, uint32_t c, uint32_t tt) {
  uint32_t r = 0;
  for (int i = 0; i < 32; ++i) r |= ((tt >> ((((a >> i) & 1u) << 2) | (((b >> i) & 1u) << 1) | ((c >> i) & 1u))) & 1u) << i;
  return r;
}
R1(bitop3_96, cro_alu_bitop3(a, b, c, 0x96))
R1(bitop3_e8, cro_alu_bitop3(a, b, c, 0xE8))
R1(bitop3_ca, cro_alu_bitop3(a, b, c, 0xCA))
R1(bitop3_1b, cro_alu_bitop3(a, b, c, 0x1B))
R1(bfrev_b32, cro_alu_rev(a))
R1(ffbh_u32, a ? cro_alu_clz(a) : ~0u)
R1(ffbl_b32, a ? cro_alu_ctz(a) : ~0u)
R1(bcnt_u32_b32, cro_alu_pop(a) + b)
R1(mbcnt_u32_b32, cro_alu_pop(0) + c)  // lane = row is filled in by cro_alu_row
// v_ashr_pk_*: both halves of the low word, the high word kept (op_sel 0)
R1(ashr_pk_i8_i32, (d & 0xFFFF0000u) | ((uint32_t)cro_alu_sat((int32_t)a >> (c & 31u), -128, 127) & 255u) | (((uint32_t)cro_alu_sat((int32_t)b >> (c & 31u), -128, 127) & 255u) << 8))
R1(ashr_pk_u8_i32, (d & 0xFFFF0000u) | (uint32_t)cro_alu_sat((int32_t)a >> (c & 31u), 0, 255) | ((uint32_t)cro_alu_sat((int32_t)b >> (c & 31u), 0, 255) << 8))
// lanes below this one whose mask bit is set, plus the base: for lane = row
// the table cannot know the lane, so cro_alu_mbcnt is what stage and tile use
CRO_COV_HD static inline uint32_t cro_alu_mbcnt(uint32_t lo, uint32_t hi, uint32_t base, uint32_t lane) {
  const uint64_t m = (((uint64_t)hi << 32) | lo) & ((1ull << lane) - 1ull);
  return cro_alu_pop(m) + base;
}
// pk_int
RH(pk_add_u16, x + y)
RH(pk_sub_i16, x - y)
RH(pk_mul_lo_u16, x * y)
RH(pk_mad_i16, (uint32_t)(SX16(x) * SX16(y) + SX16(z)))
RH(pk_mad_u16, x * y + z)
RH(pk_min_i16, SX16(x) < SX16(y) ? x : y)
RH(pk_max_i16, SX16(x) > SX16(y) ? x : y)
RH(pk_min_u16, x < y ? x : y)
RH(pk_max_u16, x > y ? x : y)
RH(pk_lshlrev_b16, y << (x & 15u))
RH(pk_ashrrev_i16, (uint32_t)(SX16(y) >> (x & 15u)))
R1(pk_add_u16_opsel, (((a >> 16) + b) & 0xFFFFu) | ((a + (b >> 16)) << 16))
R1(pk_mul_lo_u16_opsel, (((a & 0xFFFFu) * (b >> 16)) & 0xFFFFu) | (((a >> 16) * (b & 0xFFFFu)) << 16))
R1(add_u32_sdwa, (c & 0xFFFFu) | ((((a >> 16) & 255u) + (uint32_t)SX16(b)) << 16))
R1(sub_u32_sdwa, (c & 0xFFFF00FFu) | ((((a >> 16) - (b >> 24)) & 255u) << 8))
// dot
RB(dot4_i32_i8, uint32_t r = c; for (int i = 0; i < 4; ++i) r += (uint32_t)(cro_alu_sx(a >> (8 * i), 8) * cro_alu_sx(b >> (8 * i), 8)); w[0] = r;)
RB(dot4_u32_u8, uint32_t r = c; for (int i = 0; i < 4; ++i) r += ((a >> (8 * i)) & 255u) * ((b >> (8 * i)) & 255u); w[0] = r;)
RB(dot8_i32_i4, uint32_t r = c; for (int i = 0; i < 8; ++i) r += (uint32_t)(cro_alu_sx(a >> (4 * i), 4) * cro_alu_sx(b >> (4 * i), 4)); w[0] = r;)
RB(dot8_u32_u4, uint32_t r = c; for (int i = 0; i < 8; ++i) r += ((a >> (4 * i)) & 15u) * ((b >> (4 * i)) & 15u); w[0] = r;)
R1(dot2_i32_i16, (uint32_t)(SX16(a) * SX16(b)) + (uint32_t)(SX16(a >> 16) * SX16(b >> 16)) + c)
R1(dot2_u32_u16, (a & 0xFFFFu) * (b & 0xFFFFu) + (a >> 16) * (b >> 16) + c)
RF(dot2_f32_f16, HF(a) * HF(b) + HF(a >> 16) * HF(b >> 16) + (double)fc)
#define BF(v) ((double)cro_alu_f((uint32_t)(v) << 16))
RF(dot2_f32_bf16, BF(a & 0xFFFFu) * BF(b & 0xFFFFu) + BF(a >> 16) * BF(b >> 16) + (double)fc)
// f32
RF(add_f32, fa + fb)
RF(sub_f32, fa - fb)
RF(mul_f32, fa * fb)
RF(fma_f32, (double)fa * fb + fc)
RB(pk_fma_f32, w[0] = cro_alu_u((float)((double)cro_alu_f(a) * cro_alu_f(c) + cro_alu_f(e))); w[1] = cro_alu_u((float)((double)cro_alu_f(b) * cro_alu_f(d) + cro_alu_f(f)));)
RB(pk_mul_f32, w[0] = cro_alu_u(cro_alu_f(a) * cro_alu_f(c)); w[1] = cro_alu_u(cro_alu_f(b) * cro_alu_f(d));)
RB(pk_add_f32, w[0] = cro_alu_u(cro_alu_f(a) + cro_alu_f(c)); w[1] = cro_alu_u(cro_alu_f(b) + cro_alu_f(d));)
RF(add_f32_negabs, -fa + fabsf(fb))
RB(mul_f32_clamp, const float p = fa * fb; w[0] = cro_alu_u(p < 0.f ? 0.f : p > 1.f ? 1.f : p); if (p == 0.f) w[0] = 0;)
RF(fma_f32_neg, (double)fa * -(double)fb + fabs((double)fc))
// min / max order -0 below +0
static inline float cro_alu_min(float x, float y) { return x < y ? x : y < x ? y : (cro_alu_u(x) >> 31) ? x : y; }
static inline float cro_alu_max(float x, float y) { return x > y ? x : y > x ? y : (cro_alu_u(x) >> 31) ? y : x; }
RF(min_f32, cro_alu_min(fa, fb))
RF(max_f32, cro_alu_max(fa, fb))
RF(med3_f32, cro_alu_max(cro_alu_min(fa, fb), cro_alu_min(cro_alu_max(fa, fb), fc)))
RF(minimum3_f32, cro_alu_min(cro_alu_min(fa, fb), fc))
RF(maximum3_f32, cro_alu_max(cro_alu_max(fa, fb), fc))
RF(ldexp_f32, ldexp((double)fa, (int)(int32_t)b))
RB(frexp_mant_f32, int x; w[0] = cro_alu_u((float)frexp((double)fa, &x));)
RB(frexp_exp_i32_f32, int x = 0; frexp((double)fa, &x); w[0] = fa == 0.f ? 0u : (uint32_t)x;)
RB(fract_f32, const double x = (double)fa; float r = (float)(x - floor(x)); if (r >= 1.f) r = cro_alu_f(0x3F7FFFFFu); w[0] = cro_alu_u(r);)
RF(floor_f32, floorf(fa))
RF(ceil_f32, ceilf(fa))
RF(trunc_f32, truncf(fa))
RF(rndne_f32, nearbyintf(fa))
// f16
#define RHF(name, expr) static inline void cro_alu_r_##name(const uint32_t* s, uint32_t* w) { CRO_ALU_REF_HEAD \
  for (int h = 0; h < 2; ++h) { const double x = HF(a >> (16 * h)), y = HF(b >> (16 * h)), z = HF(c >> (16 * h)); \
    (void)x; (void)y; (void)z; w[0] |= cro_alu_h_of(expr) << (16 * h); } }
static inline double cro_alu_dmin(double x, double y) { return x < y ? x : y < x ? y : signbit(x) ? x : y; }
static inline double cro_alu_dmax(double x, double y) { return x > y ? x : y > x ? y : signbit(x) ? y : x; }
RHF(pk_fma_f16, x * y + z)
RHF(pk_add_f16, x + y)
RHF(pk_mul_f16, x * y)
RHF(pk_min_f16, cro_alu_dmin(x, y))
RHF(pk_max_f16, cro_alu_dmax(x, y))
// v_fma_f16 keeps the destination's high half (measured): `old` is a payload
R1(fma_f16, (d & 0xFFFF0000u) | cro_alu_h_of(HF(a) * HF(b) + HF(c)))
RF(fma_mix_f32, HF(a) * HF(b >> 16) + HF(c))
R1(fma_mixlo_f16, (d & 0xFFFF0000u) | cro_alu_h_of(HF(a >> 16) * HF(b) + HF(c >> 16)))
R1(fma_mixhi_f16, (d & 0xFFFFu) | (cro_alu_h_of(HF(a) * HF(b >> 16) + HF(c >> 16)) << 16))
// f64
RD(add_f64, da + db)
RD(mul_f64, da * db)
RD(fma_f64, da * db + dc)
RD(min_f64, cro_alu_dmin(da, db))
RD(max_f64, cro_alu_dmax(da, db))
RD(ldexp_f64, ldexp(da, (int)(int32_t)c))
RB(frexp_mant_f64, int x; cro_alu_wd(w, frexp(da, &x));)
RD(trunc_f64, trunc(da))
RD(floor_f64, floor(da))
RD(rndne_f64, nearbyint(da))
RD(div_f64, da / db)
RD(sqrt_f64, sqrt(da))
// convert
RF(cvt_f32_i32, (int32_t)a)
RF(cvt_f32_u32, a)
R1(cvt_i32_f32, fa != fa ? 0 : (int32_t)cro_alu_sat((int64_t)cro_alu_dmax(cro_alu_dmin(trunc((double)fa), 4e9), -4e9), INT32_MIN, INT32_MAX))
R1(cvt_u32_f32, fa != fa ? 0 : (uint32_t)cro_alu_sat((int64_t)cro_alu_dmax(cro_alu_dmin(trunc((double)fa), 8e9), -8e9), 0, 0xFFFFFFFFll))
R1(cvt_f16_f32, cro_alu_h_of((double)fa))
RF(cvt_f32_f16, HF(a))
R1(cvt_pkrtz_f16_f32, cro_alu_h_of((double)fa, 1) | (cro_alu_h_of((double)fb, 1) << 16))
R1(cvt_pk_bf16_f32, cro_alu_bf16_of(a) | (cro_alu_bf16_of(b) << 16))
RB(cvt_f64_f32, cro_alu_wd(w, (double)fa);)
RF(cvt_f32_f64, da)
RB(cvt_f64_i32, cro_alu_wd(w, (double)(int32_t)a);)
R1(cvt_i32_f64, (int32_t)cro_alu_sat((int64_t)cro_alu_dmax(cro_alu_dmin(trunc(da), 4e9), -4e9), INT32_MIN, INT32_MAX))
RF(cvt_f32_ubyte0, a & 255u)
RF(cvt_f32_ubyte1, (a >> 8) & 255u)
RF(cvt_f32_ubyte2, (a >> 16) & 255u)
RF(cvt_f32_ubyte3, a >> 24)
R1(cvt_pk_i16_i32, ((uint32_t)cro_alu_sat((int32_t)a, -32768, 32767) & 0xFFFFu) | ((uint32_t)cro_alu_sat((int32_t)b, -32768, 32767) << 16))
R1(cvt_pk_u16_u32, (a > 0xFFFFu ? 0xFFFFu : a) | ((b > 0xFFFFu ? 0xFFFFu : b) << 16))
R1(cvt_pk_u8_f32, fa != fa ? (c & ~(255u << (8u * (b & 3u)))) : (c & ~(255u << (8u * (b & 3u)))) | ((uint32_t)cro_alu_sat((int64_t)nearbyint(cro_alu_dmax(cro_alu_dmin((double)fa, 1e6), -1e6)), 0, 255) << (8u * (b & 3u))))
static inline uint32_t cro_alu_snorm16(float x) {
  const double v = x < -1.f ? -1.0 : x > 1.f ? 1.0 : (double)x;
  return (uint32_t)(int32_t)nearbyint(v * 32767.0) & 0xFFFFu;
}
R1(cvt_pknorm_i16_f32, cro_alu_snorm16(fa) | (cro_alu_snorm16(fb) << 16))
// scale_convert: value = code value * scale; codes from croformats.h
static inline uint32_t cro_alu_dec(int fmt, uint32_t code, float scale) { return cro_alu_u((float)(cro_fmt_decode(fmt, code) * (double)scale)); }
// The code x / scale rounds to, as the device does it (measured through the
// tile entry): the nearest code of the format read as a plain minifloat
// without specials (ties to the even code), saturating at max_code: e4m3
// 0x7F (the NaN code: what overflow gives), e5m2 0x7C (the infinity code),
// e2m1 7 (its largest value)
static inline uint32_t cro_alu_encd(int fmt, double x, float scale, uint32_t max_code);
static inline uint32_t cro_alu_enc(int fmt, float x, float scale, uint32_t max_code) {
  return cro_alu_encd(fmt, (double)x, scale, max_code);
}
static inline uint32_t cro_alu_encd(int fmt, double x, float scale, uint32_t max_code) {
  const int eb = fmt == CRO_FMT_E4M3 ? 4 : fmt == CRO_FMT_E5M2 ? 5 : 2;
  const int mb = fmt == CRO_FMT_E4M3 ? 3 : fmt == CRO_FMT_E5M2 ? 2 : 1;
  const int bias = fmt == CRO_FMT_E4M3 ? 7 : fmt == CRO_FMT_E5M2 ? 15 : 1;
  const double v = fabs(x / (double)scale);
  const uint32_t sign = (uint32_t)(signbit(x) ? 1 : 0) << (cro_fmt_bits(fmt) - 1);
  uint32_t best = 0;
  for (uint32_t k = 0; k <= max_code; ++k) {
    const double lo = cro_fmt_minifloat(best, eb, mb, bias), hi = cro_fmt_minifloat(k, eb, mb, bias);
    if (fabs(hi - v) < fabs(lo - v) || (fabs(hi - v) == fabs(lo - v) && !(k & 1u))) best = k;
  }
  return sign | best;
}
RB(sc_pk_f32_fp8, w[0] = cro_alu_dec(CRO_FMT_E4M3, a & 255u, fb); w[1] = cro_alu_dec(CRO_FMT_E4M3, (a >> 8) & 255u, fb);)
RB(sc_pk_f32_fp8_hi, w[0] = cro_alu_dec(CRO_FMT_E4M3, (a >> 16) & 255u, fb); w[1] = cro_alu_dec(CRO_FMT_E4M3, a >> 24, fb);)
RB(sc_pk_f32_bf8, w[0] = cro_alu_dec(CRO_FMT_E5M2, a & 255u, fb); w[1] = cro_alu_dec(CRO_FMT_E5M2, (a >> 8) & 255u, fb);)
RB(sc_pk_f32_fp4, w[0] = cro_alu_dec(CRO_FMT_E2M1, a & 15u, fb); w[1] = cro_alu_dec(CRO_FMT_E2M1, (a >> 4) & 15u, fb);)
R1(sc_pk_fp8_f32, (d & 0xFFFF0000u) | cro_alu_enc(CRO_FMT_E4M3, fa, fc, 0x7F) | (cro_alu_enc(CRO_FMT_E4M3, fb, fc, 0x7F) << 8))
R1(sc_pk_fp8_f32_hi, (d & 0xFFFFu) | (cro_alu_enc(CRO_FMT_E4M3, fa, fc, 0x7F) << 16) | (cro_alu_enc(CRO_FMT_E4M3, fb, fc, 0x7F) << 24))
R1(sc_pk_bf8_f32, (d & 0xFFFF0000u) | cro_alu_enc(CRO_FMT_E5M2, fa, fc, 0x7C) | (cro_alu_enc(CRO_FMT_E5M2, fb, fc, 0x7C) << 8))
R1(sc_pk_fp4_f32, (d & 0xFFFFFF00u) | cro_alu_enc(CRO_FMT_E2M1, fa, fc, 7) | (cro_alu_enc(CRO_FMT_E2M1, fb, fc, 7) << 4))
// element i is bits 6i+5..6i of the 192-bit operand
static inline void cro_alu_fp6_fold(const uint32_t* s, float scale, uint32_t* w) {
  w[0] = w[1] = 0;
  for (int i = 0; i < 32; ++i) {
    const int bit = 6 * i;
    uint32_t code = s[bit >> 5] >> (bit & 31);
    if ((bit & 31) > 26) code |= s[(bit >> 5) + 1] << (32 - (bit & 31));
    const uint32_t v = cro_alu_dec(CRO_FMT_E2M3, code & 63u, scale);
    w[i & 1] = ((w[i & 1] << 5) | (w[i & 1] >> 27)) ^ v;
  }
}
RB(sc_pk32_f32_fp6_x2, cro_alu_fp6_fold(s, 2.0f, w);)
RB(sc_pk32_f32_fp6_half, cro_alu_fp6_fold(s, 0.5f, w);)
R1(sc_pk_fp8_f16, (c & 0xFFFF0000u) | cro_alu_encd(CRO_FMT_E4M3, HF(a), fb, 0x7F) | (cro_alu_encd(CRO_FMT_E4M3, HF(a >> 16), fb, 0x7F) << 8))
R1(sc_pk_fp8_bf16, (c & 0xFFFF0000u) | cro_alu_encd(CRO_FMT_E4M3, (double)cro_alu_f((a & 0xFFFFu) << 16), fb, 0x7F) | (cro_alu_encd(CRO_FMT_E4M3, (double)cro_alu_f(a & 0xFFFF0000u), fb, 0x7F) << 8))
// compare_select: 1 where the predicate holds.  Predicate codes: bit 0 <,
// bit 1 ==, bit 2 >, bit 3 unordered.
static inline uint32_t cro_alu_rel(double x, double y) { return x != x || y != y ? 8u : x < y ? 1u : x == y ? 2u : 4u; }
static inline uint32_t cro_alu_reli(int64_t x, int64_t y) { return x < y ? 1u : x == y ? 2u : 4u; }
static inline uint32_t cro_alu_relu(uint64_t x, uint64_t y) { return x < y ? 1u : x == y ? 2u : 4u; }
#define CRO_ALU_P_lt 1u
#define CRO_ALU_P_eq 2u
#define CRO_ALU_P_le 3u
#define CRO_ALU_P_gt 4u
#define CRO_ALU_P_lg 5u
#define CRO_ALU_P_ne 13u
#define CRO_ALU_P_ge 6u
#define CRO_ALU_P_o 7u
#define CRO_ALU_P_u 8u
#define CRO_ALU_P_nge 9u
#define CRO_ALU_P_nlt 14u
#define RCF32(p) R1(cmp_##p##_f32, (cro_alu_rel(fa, fb) & CRO_ALU_P_##p) != 0)
#define RCF64(p) R1(cmp_##p##_f64, (cro_alu_rel(da, db) & CRO_ALU_P_##p) != 0)
#define RCF16(p) R1(cmp_##p##_f16, (cro_alu_rel(HF(a), HF(b)) & CRO_ALU_P_##p) != 0)
#define RCI(p) R1(cmp_##p##_i32, (cro_alu_reli((int32_t)a, (int32_t)b) & CRO_ALU_P_##p) != 0) \
  R1(cmp_##p##_u32, (cro_alu_relu(a, b) & CRO_ALU_P_##p) != 0) \
  R1(cmp_##p##_i64, (cro_alu_reli((int64_t)A, (int64_t)B) & CRO_ALU_P_##p) != 0) \
  R1(cmp_##p##_u64, (cro_alu_relu(A, B) & CRO_ALU_P_##p) != 0)
RCF32(lt) RCF32(le) RCF32(eq) RCF32(lg) RCF32(gt) RCF32(ge) RCF32(o) RCF32(u) RCF32(nge) RCF32(nlt)
RCF64(lt) RCF64(le) RCF64(eq) RCF64(lg) RCF64(gt) RCF64(ge)
RCF16(lt) RCF16(le) RCF16(eq) RCF16(lg) RCF16(gt) RCF16(ge)
RCI(lt) RCI(eq) RCI(gt) RCI(ne)
// class bits: 0 sNaN 1 qNaN 2 -inf 3 -normal 4 -subnormal 5 -0 6 +0 7 +subnormal 8 +normal 9 +inf
static inline uint32_t cro_alu_class(uint64_t bits, int ebits, int mbits) {
  const uint64_t m = bits & ((1ull << mbits) - 1), ex = (bits >> mbits) & ((1ull << ebits) - 1);
  const bool neg = (bits >> (ebits + mbits)) & 1;
  if (ex == (1ull << ebits) - 1) return m ? ((m >> (mbits - 1)) ? 1u : 0u) : neg ? 2u : 9u;
  if (ex) return neg ? 3u : 8u;
  if (m) return neg ? 4u : 7u;
  return neg ? 5u : 6u;
}
R1(cmp_class_f32, (b >> cro_alu_class(a, 8, 23)) & 1u)
R1(cmp_class_f64, (c >> cro_alu_class(A, 11, 52)) & 1u)
R1(cmpx_lt_u32, a < b ? a : c)
// salu (the second word of an S1C form is SCC)
RB(s_add_u64, cro_alu_w64(w, (((uint64_t)c << 32) | a) + (((uint64_t)d << 32) | b));)
RB(s_sub_u64, cro_alu_w64(w, (((uint64_t)c << 32) | a) - (((uint64_t)d << 32) | b));)
R1(s_mul_i32, a * b)
R1(s_mul_hi_u32, ((uint64_t)a * b) >> 32)
R1(s_mul_hi_i32, (uint64_t)((int64_t)(int32_t)a * (int32_t)b) >> 32)
#define RSC(name, expr) RB(name, w[0] = (uint32_t)(expr); w[1] = w[0] != 0;)
RSC(s_lshl_b32, a << (b & 31u))
RSC(s_lshr_b32, a >> (b & 31u))
RSC(s_ashr_i32, (int32_t)a >> (b & 31u))
R2(s_lshl_b64, A << (c & 63u))
R2(s_lshr_b64, A >> (c & 63u))
R2(s_ashr_i64, (int64_t)A >> (c & 63u))
RSC(s_and_b32, a & b) RSC(s_or_b32, a | b) RSC(s_xor_b32, a ^ b) RSC(s_nand_b32, ~(a & b))
RSC(s_nor_b32, ~(a | b)) RSC(s_xnor_b32, ~(a ^ b)) RSC(s_andn2_b32, a & ~b) RSC(s_orn2_b32, a | ~b)
R2(s_and_b64, A & B) R2(s_or_b64, A | B) R2(s_xor_b64, A ^ B) R2(s_nand_b64, ~(A & B))
R2(s_nor_b64, ~(A | B)) R2(s_xnor_b64, ~(A ^ B)) R2(s_andn2_b64, A & ~B) R2(s_orn2_b64, A | ~B)
RSC(s_not_b32, ~a)
R1(s_brev_b32, cro_alu_rev(a))
R2(s_brev_b64, ((uint64_t)cro_alu_rev(a) << 32) | cro_alu_rev(b))
RSC(s_bcnt0_i32_b32, 32u - cro_alu_pop(a))
RSC(s_bcnt1_i32_b64, cro_alu_pop(A))
R1(s_ff0_i32_b32, ~a ? cro_alu_ctz(~a) : ~0u)
R1(s_ff1_i32_b32, a ? cro_alu_ctz(a) : ~0u)
R1(s_ff1_i32_b64, a ? cro_alu_ctz(a) : b ? 32u + cro_alu_ctz(b) : ~0u)
R1(s_flbit_i32_b32, a ? cro_alu_clz(a) : ~0u)
R1(s_flbit_i32, (a == 0u || a == ~0u) ? ~0u : cro_alu_clz((a >> 31) ? ~a : a))
R1(s_flbit_i32_b64, b ? cro_alu_clz(b) : a ? 32u + cro_alu_clz(a) : ~0u)
R1(s_sext_i32_i8, cro_alu_sx(a, 8))
R1(s_sext_i32_i16, cro_alu_sx(a, 16))
R1(s_bfm_b32, ((1u << (a & 31u)) - 1u) << (b & 31u))
RB(s_bfe_u32, const uint32_t o = b & 31u, n = (b >> 16) & 127u; w[0] = !n ? 0u : n >= 32 ? a >> o : (a >> o) & ((1u << n) - 1u); w[1] = w[0] != 0;)
RB(s_bfe_i32, const uint32_t o = b & 31u, n = (b >> 16) & 127u;
   w[0] = !n ? 0u : o + n < 32 ? (uint32_t)((int32_t)(a << (32 - o - n)) >> (32 - n)) : (uint32_t)((int32_t)a >> o); w[1] = w[0] != 0;)
static inline uint64_t cro_alu_bfe64(uint64_t v, uint32_t sel, bool sign) {
  const uint32_t o = sel & 63u, n = (sel >> 16) & 127u;
  if (!n) return 0;
  if (o + n >= 64) return sign ? (uint64_t)((int64_t)v >> o) : v >> o;
  return sign ? (uint64_t)((int64_t)(v << (64 - o - n)) >> (64 - n)) : (v >> o) & ((1ull << n) - 1ull);
}
R2(s_bfe_u64, cro_alu_bfe64(A, c, false))
R2(s_bfe_i64, cro_alu_bfe64(A, c, true))
// SCC of the forms whose result fills both words
#define RNZ(name, expr) R1(name##_scc, (uint64_t)(expr) != 0)
RNZ(s_and_b64, A & B) RNZ(s_or_b64, A | B) RNZ(s_xor_b64, A ^ B) RNZ(s_nand_b64, ~(A & B))
RNZ(s_nor_b64, ~(A | B)) RNZ(s_xnor_b64, ~(A ^ B)) RNZ(s_andn2_b64, A & ~B) RNZ(s_orn2_b64, A | ~B)
RNZ(s_lshl_b64, A << (c & 63u)) RNZ(s_lshr_b64, A >> (c & 63u)) RNZ(s_ashr_i64, (int64_t)A >> (c & 63u))
RNZ(s_bfe_u64, cro_alu_bfe64(A, c, false)) RNZ(s_bfe_i64, cro_alu_bfe64(A, c, true))
// the carry out of the high add, the borrow out of the high subtract
RB(s_add_u64_scc, const uint64_t x = ((uint64_t)c << 32) | a, y = ((uint64_t)d << 32) | b; w[0] = x + y < x;)
RB(s_sub_u64_scc, const uint64_t x = ((uint64_t)c << 32) | a, y = ((uint64_t)d << 32) | b; w[0] = x < y;)
#define RSEL(name, cond) R1(name, (cond) ? c : d)
RSEL(s_cselect_eq_i32, a == b) RSEL(s_cselect_lg_i32, a != b)
RSEL(s_cselect_lt_i32, (int32_t)a < (int32_t)b) RSEL(s_cselect_gt_i32, (int32_t)a > (int32_t)b)
RSEL(s_cselect_eq_u32, a == b) RSEL(s_cselect_lg_u32, a != b) RSEL(s_cselect_lt_u32, a < b) RSEL(s_cselect_gt_u32, a > b)
// the difference wraps before its magnitude is taken
RSC(s_absdiff_i32, ((a - b) >> 31) ? b - a : a - b)
RB(s_min_i32, const bool t = (int32_t)a < (int32_t)b; w[0] = t ? a : b; w[1] = t;)
RB(s_max_u32, const bool t = a > b; w[0] = t ? a : b; w[1] = t;)
#define RSLA(n) RB(s_lshl##n##_add_u32, const uint64_t t = ((uint64_t)a << n) + b; w[0] = (uint32_t)t; w[1] = t >> 32 ? 1u : 0u;)
RSLA(1) RSLA(2) RSLA(3) RSLA(4)
R1(s_pack_ll_b32_b16, (a & 0xFFFFu) | (b << 16))
R1(s_pack_lh_b32_b16, (a & 0xFFFFu) | (b & 0xFFFF0000u))
R1(s_pack_hh_b32_b16, (a >> 16) | (b & 0xFFFF0000u))
// transcendental: what an anchor row must give (the other rows' expected
// words are never compared: cro_alu_row zeroes them)
RF(t_exp_f32, exp2((double)fa))
RF(t_log_f32, log2((double)fa))
RF(t_rcp_f32, 1.0 / (double)fa)
RF(t_rsq_f32, 1.0 / sqrt((double)fa))
RF(t_sqrt_f32, sqrt((double)fa))
// the argument is in revolutions; exact at the multiples of a quarter
static inline double cro_alu_sinrev(double x) {
  const double q = 4.0 * x;
  if (q == floor(q)) { static const double v[4] = {0.0, 1.0, 0.0, -1.0}; return v[(int)(q - 4.0 * floor(q / 4.0))]; }
  return sin(6.283185307179586 * x);
}
RF(t_sin_f32, cro_alu_sinrev((double)fa))
RF(t_cos_f32, cro_alu_sinrev((double)fa + 0.25))
RD(t_rcp_f64, 1.0 / da)
RD(t_rsq_f64, 1.0 / sqrt(da))
RD(t_sqrt_f64, sqrt(da))
R1(t_exp_f16, cro_alu_h_of(exp2(HF(a))))
R1(t_log_f16, cro_alu_h_of(log2(HF(a))))
R1(t_rcp_f16, cro_alu_h_of(1.0 / HF(a)))
R1(t_sqrt_f16, cro_alu_h_of(sqrt(HF(a))))

// -- the form list ---------------------------------------------------------------------
// X(check, name, mnemonic, asm template, signature, operand class).  %0 is
// the result (%0, %1 where the signature has two separate result registers),
// the sources follow in order.  The reference is cro_alu_r_<name>.
#define CMPT(op) op " vcc, %1, %2\n\ts_nop 4\n\tv_cndmask_b32_e64 %0, 0, 1, vcc"
#define CRO_ALU_XCMPF(X, p) X(CMP, cmp_##p##_f32, "v_cmp_" #p "_f32", CMPT("v_cmp_" #p "_f32"), V1_VV, CMPF32)
#define CRO_ALU_XCMPD(X, p) X(CMP, cmp_##p##_f64, "v_cmp_" #p "_f64", CMPT("v_cmp_" #p "_f64"), V1_DD, CMPF64)
#define CRO_ALU_XCMPH(X, p) X(CMP, cmp_##p##_f16, "v_cmp_" #p "_f16", CMPT("v_cmp_" #p "_f16"), V1_VV, CMPF16)
#define CRO_ALU_XCMPI(X, p)                                                                      \
  X(CMP, cmp_##p##_i32, "v_cmp_" #p "_i32", CMPT("v_cmp_" #p "_i32"), V1_VV, CMPINT)              \
  X(CMP, cmp_##p##_u32, "v_cmp_" #p "_u32", CMPT("v_cmp_" #p "_u32"), V1_VV, CMPINT)              \
  X(CMP, cmp_##p##_i64, "v_cmp_" #p "_i64", CMPT("v_cmp_" #p "_i64"), V1_DD, CMPINT)              \
  X(CMP, cmp_##p##_u64, "v_cmp_" #p "_u64", CMPT("v_cmp_" #p "_u64"), V1_DD, CMPINT)
#define CRO_ALU_XS2(X, op) X(SALU, op, #op, #op " %0, %1, %2", S1_SS, INT)
#define CRO_ALU_XS2C(X, op) X(SALU, op, #op, #op " %0, %2, %3\n\ts_cselect_b32 %1, 1, 0", S1C_SS, INT)
#define CRO_ALU_XS64(X, op) X(SALU, op, #op, #op " %0, %1, %2", S2_QQ, INT)
#define CRO_ALU_XSCQ(X, op, sig) X(SALU, op##_scc, #op, #op " %1, %2, %3\n\ts_cselect_b32 %0, 1, 0", sig, INT)
#define CRO_ALU_XSEL(X, p, t)                                                                    \
  X(SALU, s_cselect_##p##_##t, "s_cmp_" #p "_" #t, "s_cmp_" #p "_" #t " %1, %2\n\ts_cselect_b32 %0, %3, %4", S1_SSSS, CMPINT)
#define CRO_ALU_XT(X, op, sig, cls) X(TRANS, t_##op, "v_" #op, "v_" #op " %0, %1", sig, cls)

#define CRO_ALU_FORMS(X)                                                                         \
  X(INT, add_u64, "v_addc_co_u32", "v_add_co_u32 %0, vcc, %2, %4\n\tv_addc_co_u32 %1, vcc, %3, %5, vcc", V2C_VVVV, INT) \
  X(INT, sub_u64, "v_subb_co_u32", "v_sub_co_u32 %0, vcc, %2, %4\n\tv_subb_co_u32 %1, vcc, %3, %5, vcc", V2C_VVVV, INT) \
  X(INT, mul_lo_u32, "v_mul_lo_u32", "v_mul_lo_u32 %0, %1, %2", V1_VV, INT)                      \
  X(INT, mul_hi_u32, "v_mul_hi_u32", "v_mul_hi_u32 %0, %1, %2", V1_VV, INT)                      \
  X(INT, mul_hi_i32, "v_mul_hi_i32", "v_mul_hi_i32 %0, %1, %2", V1_VV, INT)                      \
  X(INT, mad_u64_u32, "v_mad_u64_u32", "v_mad_u64_u32 %0, vcc, %1, %2, %3", V2_VVD, INT)         \
  X(INT, mad_i64_i32, "v_mad_i64_i32", "v_mad_i64_i32 %0, vcc, %1, %2, %3", V2_VVD, INT)         \
  X(INT, mad_u32_u24, "v_mad_u32_u24", "v_mad_u32_u24 %0, %1, %2, %3", V1_VVV, INT)              \
  X(INT, mul_i32_i24, "v_mul_i32_i24", "v_mul_i32_i24 %0, %1, %2", V1_VV, INT)                   \
  X(INT, lshl_add_u32, "v_lshl_add_u32", "v_lshl_add_u32 %0, %1, %2, %3", V1_VVV, INT)           \
  X(INT, add3_u32, "v_add3_u32", "v_add3_u32 %0, %1, %2, %3", V1_VVV, INT)                       \
  X(INT, sad_u8, "v_sad_u8", "v_sad_u8 %0, %1, %2, %3", V1_VVV, INT)                             \
  X(BIT, lshlrev_b32, "v_lshlrev_b32", "v_lshlrev_b32 %0, %1, %2", V1_VV, INT)                   \
  X(BIT, lshrrev_b32, "v_lshrrev_b32", "v_lshrrev_b32 %0, %1, %2", V1_VV, INT)                   \
  X(BIT, ashrrev_i32, "v_ashrrev_i32", "v_ashrrev_i32 %0, %1, %2", V1_VV, INT)                   \
  X(BIT, lshlrev_b64, "v_lshlrev_b64", "v_lshlrev_b64 %0, %1, %2", V2_VD, INT)                   \
  X(BIT, lshrrev_b64, "v_lshrrev_b64", "v_lshrrev_b64 %0, %1, %2", V2_VD, INT)                   \
  X(BIT, ashrrev_i64, "v_ashrrev_i64", "v_ashrrev_i64 %0, %1, %2", V2_VD, INT)                   \
  X(BIT, bfe_u32, "v_bfe_u32", "v_bfe_u32 %0, %1, %2, %3", V1_VVV, INT)                          \
  X(BIT, bfe_i32, "v_bfe_i32", "v_bfe_i32 %0, %1, %2, %3", V1_VVV, INT)                          \
  X(BIT, bfi_b32, "v_bfi_b32", "v_bfi_b32 %0, %1, %2, %3", V1_VVV, INT)                          \
  X(BIT, alignbit_b32, "v_alignbit_b32", "v_alignbit_b32 %0, %1, %2, %3", V1_VVV, INT)           \
  X(BIT, alignbyte_b32, "v_alignbyte_b32", "v_alignbyte_b32 %0, %1, %2, %3", V1_VVV, INT)        \
  X(BIT, perm_b32, "v_perm_b32", "v_perm_b32 %0, %1, %2, %3", V1_VVV, PERM)                       \
  X(BIT, bitop3_96, "v_bitop3_b32", "v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96", V1_VVV, INT)      \
  X(BIT, bitop3_e8, "v_bitop3_b32", "v_bitop3_b32 %0, %1, %2, %3 bitop3:0xe8", V1_VVV, INT)      \
  X(BIT, bitop3_ca, "v_bitop3_b32", "v_bitop3_b32 %0, %1, %2, %3 bitop3:0xca", V1_VVV, INT)      \
  X(BIT, bitop3_1b, "v_bitop3_b32", "v_bitop3_b32 %0, %1, %2, %3 bitop3:0x1b", V1_VVV, INT)      \
  X(BIT, bfrev_b32, "v_bfrev_b32", "v_bfrev_b32 %0, %1", V1_V, INT)                              \
  X(BIT, ffbh_u32, "v_ffbh_u32", "v_ffbh_u32 %0, %1", V1_V, INT)                                 \
  X(BIT, ffbl_b32, "v_ffbl_b32", "v_ffbl_b32 %0, %1", V1_V, INT)                                 \
  X(BIT, bcnt_u32_b32, "v_bcnt_u32_b32", "v_bcnt_u32_b32 %0, %1, %2", V1_VV, INT)                \
  X(BIT, mbcnt_u32_b32, "v_mbcnt_hi_u32_b32", "v_mbcnt_lo_u32_b32 %0, %1, %3\n\tv_mbcnt_hi_u32_b32 %0, %2, %0", V1_MBCNT, INT) \
  X(BIT, ashr_pk_i8_i32, "v_ashr_pk_i8_i32", "v_ashr_pk_i8_i32 %0, %1, %2, %3", V1_VVVO, INT)    \
  X(BIT, ashr_pk_u8_i32, "v_ashr_pk_u8_i32", "v_ashr_pk_u8_i32 %0, %1, %2, %3", V1_VVVO, INT)    \
  X(PKINT, pk_add_u16, "v_pk_add_u16", "v_pk_add_u16 %0, %1, %2", V1_VV, INT)                    \
  X(PKINT, pk_sub_i16, "v_pk_sub_i16", "v_pk_sub_i16 %0, %1, %2", V1_VV, INT)                    \
  X(PKINT, pk_mul_lo_u16, "v_pk_mul_lo_u16", "v_pk_mul_lo_u16 %0, %1, %2", V1_VV, INT)           \
  X(PKINT, pk_mad_i16, "v_pk_mad_i16", "v_pk_mad_i16 %0, %1, %2, %3", V1_VVV, INT)               \
  X(PKINT, pk_mad_u16, "v_pk_mad_u16", "v_pk_mad_u16 %0, %1, %2, %3", V1_VVV, INT)               \
  X(PKINT, pk_min_i16, "v_pk_min_i16", "v_pk_min_i16 %0, %1, %2", V1_VV, INT)                    \
  X(PKINT, pk_max_i16, "v_pk_max_i16", "v_pk_max_i16 %0, %1, %2", V1_VV, INT)                    \
  X(PKINT, pk_min_u16, "v_pk_min_u16", "v_pk_min_u16 %0, %1, %2", V1_VV, INT)                    \
  X(PKINT, pk_max_u16, "v_pk_max_u16", "v_pk_max_u16 %0, %1, %2", V1_VV, INT)                    \
  X(PKINT, pk_lshlrev_b16, "v_pk_lshlrev_b16", "v_pk_lshlrev_b16 %0, %1, %2", V1_VV, INT)        \
  X(PKINT, pk_ashrrev_i16, "v_pk_ashrrev_i16", "v_pk_ashrrev_i16 %0, %1, %2", V1_VV, INT)        \
  X(PKINT, pk_add_u16_opsel, "v_pk_add_u16", "v_pk_add_u16 %0, %1, %2 op_sel:[1,0] op_sel_hi:[0,1]", V1_VV, INT) \
  X(PKINT, pk_mul_lo_u16_opsel, "v_pk_mul_lo_u16", "v_pk_mul_lo_u16 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0]", V1_VV, INT) \
  X(PKINT, add_u32_sdwa, "v_add_u32_sdwa", "v_add_u32_sdwa %0, %1, sext(%2) dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_2 src1_sel:WORD_0", V1_VVO, INT) \
  X(PKINT, sub_u32_sdwa, "v_sub_u32_sdwa", "v_sub_u32_sdwa %0, %1, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:BYTE_3", V1_VVO, INT) \
  X(DOT, dot4_i32_i8, "v_dot4_i32_i8", "v_dot4_i32_i8 %0, %1, %2, %3", V1_VVV, INT)              \
  X(DOT, dot4_u32_u8, "v_dot4_u32_u8", "v_dot4_u32_u8 %0, %1, %2, %3", V1_VVV, INT)              \
  X(DOT, dot8_i32_i4, "v_dot8_i32_i4", "v_dot8_i32_i4 %0, %1, %2, %3", V1_VVV, INT)              \
  X(DOT, dot8_u32_u4, "v_dot8_u32_u4", "v_dot8_u32_u4 %0, %1, %2, %3", V1_VVV, INT)              \
  X(DOT, dot2_i32_i16, "v_dot2_i32_i16", "v_dot2_i32_i16 %0, %1, %2, %3", V1_VVV, INT)           \
  X(DOT, dot2_u32_u16, "v_dot2_u32_u16", "v_dot2_u32_u16 %0, %1, %2, %3", V1_VVV, INT)           \
  X(DOT, dot2_f32_f16, "v_dot2_f32_f16", "v_dot2_f32_f16 %0, %1, %2, %3", V1_VVV, DOTF16)        \
  X(DOT, dot2_f32_bf16, "v_dot2_f32_bf16", "v_dot2_f32_bf16 %0, %1, %2, %3", V1_VVV, DOTBF16)    \
  X(F32, add_f32, "v_add_f32", "v_add_f32 %0, %1, %2", V1_VV, F32)                               \
  X(F32, sub_f32, "v_sub_f32", "v_sub_f32 %0, %1, %2", V1_VV, F32)                               \
  X(F32, mul_f32, "v_mul_f32", "v_mul_f32 %0, %1, %2", V1_VV, F32)                               \
  X(F32, fma_f32, "v_fma_f32", "v_fma_f32 %0, %1, %2, %3", V1_VVV, F32FMA)                       \
  X(F32, pk_fma_f32, "v_pk_fma_f32", "v_pk_fma_f32 %0, %1, %2, %3", V2_DDD, F32PKFMA)            \
  X(F32, pk_mul_f32, "v_pk_mul_f32", "v_pk_mul_f32 %0, %1, %2", V2_DD, F32)                      \
  X(F32, pk_add_f32, "v_pk_add_f32", "v_pk_add_f32 %0, %1, %2", V2_DD, F32)                      \
  X(F32, add_f32_negabs, "v_add_f32", "v_add_f32_e64 %0, -%1, |%2|", V1_VV, F32)                 \
  X(F32, mul_f32_clamp, "v_mul_f32", "v_mul_f32_e64 %0, %1, %2 clamp", V1_VV, F32)               \
  X(F32, fma_f32_neg, "v_fma_f32", "v_fma_f32 %0, %1, -%2, |%3|", V1_VVV, F32FMA)                \
  X(F32, min_f32, "v_min_f32", "v_min_f32 %0, %1, %2", V1_VV, F32)                               \
  X(F32, max_f32, "v_max_f32", "v_max_f32 %0, %1, %2", V1_VV, F32)                               \
  X(F32, med3_f32, "v_med3_f32", "v_med3_f32 %0, %1, %2, %3", V1_VVV, F32)                       \
  X(F32, minimum3_f32, "v_minimum3_f32", "v_minimum3_f32 %0, %1, %2, %3", V1_VVV, F32)           \
  X(F32, maximum3_f32, "v_maximum3_f32", "v_maximum3_f32 %0, %1, %2, %3", V1_VVV, F32)           \
  X(F32, ldexp_f32, "v_ldexp_f32", "v_ldexp_f32 %0, %1, %2", V1_VV, F32I)                        \
  X(F32, frexp_mant_f32, "v_frexp_mant_f32", "v_frexp_mant_f32 %0, %1", V1_V, F32)               \
  X(F32, frexp_exp_i32_f32, "v_frexp_exp_i32_f32", "v_frexp_exp_i32_f32 %0, %1", V1_V, F32)      \
  X(F32, fract_f32, "v_fract_f32", "v_fract_f32 %0, %1", V1_V, F32)                              \
  X(F32, floor_f32, "v_floor_f32", "v_floor_f32 %0, %1", V1_V, F32)                              \
  X(F32, ceil_f32, "v_ceil_f32", "v_ceil_f32 %0, %1", V1_V, F32)                                 \
  X(F32, trunc_f32, "v_trunc_f32", "v_trunc_f32 %0, %1", V1_V, F32)                              \
  X(F32, rndne_f32, "v_rndne_f32", "v_rndne_f32 %0, %1", V1_V, F32)                              \
  X(F16, pk_fma_f16, "v_pk_fma_f16", "v_pk_fma_f16 %0, %1, %2, %3", V1_VVV, F16FMA)              \
  X(F16, pk_add_f16, "v_pk_add_f16", "v_pk_add_f16 %0, %1, %2", V1_VV, F16)                      \
  X(F16, pk_mul_f16, "v_pk_mul_f16", "v_pk_mul_f16 %0, %1, %2", V1_VV, F16)                      \
  X(F16, pk_min_f16, "v_pk_min_f16", "v_pk_min_f16 %0, %1, %2", V1_VV, F16)                      \
  X(F16, pk_max_f16, "v_pk_max_f16", "v_pk_max_f16 %0, %1, %2", V1_VV, F16)                      \
  X(F16, fma_f16, "v_fma_f16", "v_fma_f16 %0, %1, %2, %3", V1_VVVO, F16FMA)                       \
  X(F16, fma_mix_f32, "v_fma_mix_f32", "v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]", V1_VVV, F16FMA) \
  X(F16, fma_mixlo_f16, "v_fma_mixlo_f16", "v_fma_mixlo_f16 %0, %1, %2, %3 op_sel:[1,0,1] op_sel_hi:[1,1,1]", V1_VVVO, F16FMA) \
  X(F16, fma_mixhi_f16, "v_fma_mixhi_f16", "v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[0,1,1] op_sel_hi:[1,1,1]", V1_VVVO, F16FMA) \
  X(F64, add_f64, "v_add_f64", "v_add_f64 %0, %1, %2", V2_DD, F64)                               \
  X(F64, mul_f64, "v_mul_f64", "v_mul_f64 %0, %1, %2", V2_DD, F64)                               \
  X(F64, fma_f64, "v_fma_f64", "v_fma_f64 %0, %1, %2, %3", V2_DDD, F64FMA)                       \
  X(F64, min_f64, "v_min_f64", "v_min_f64 %0, %1, %2", V2_DD, F64)                               \
  X(F64, max_f64, "v_max_f64", "v_max_f64 %0, %1, %2", V2_DD, F64)                               \
  X(F64, ldexp_f64, "v_ldexp_f64", "v_ldexp_f64 %0, %1, %2", V2_DV, F64I)                        \
  X(F64, frexp_mant_f64, "v_frexp_mant_f64", "v_frexp_mant_f64 %0, %1", V2_D, F64R)              \
  X(F64, trunc_f64, "v_trunc_f64", "v_trunc_f64 %0, %1", V2_D, F64R)                             \
  X(F64, floor_f64, "v_floor_f64", "v_floor_f64 %0, %1", V2_D, F64R)                             \
  X(F64, rndne_f64, "v_rndne_f64", "v_rndne_f64 %0, %1", V2_D, F64R)                             \
  X(F64, div_f64, "v_div_fixup_f64", "", X_DIV, F64DIV)                                            \
  X(F64, sqrt_f64, "v_rsq_f64", "", X_SQRT, F64DIV)                                                \
  X(CVT, cvt_f32_i32, "v_cvt_f32_i32", "v_cvt_f32_i32 %0, %1", V1_V, INT)                        \
  X(CVT, cvt_f32_u32, "v_cvt_f32_u32", "v_cvt_f32_u32 %0, %1", V1_V, INT)                        \
  X(CVT, cvt_i32_f32, "v_cvt_i32_f32", "v_cvt_i32_f32 %0, %1", V1_V, F32CVT)                     \
  X(CVT, cvt_u32_f32, "v_cvt_u32_f32", "v_cvt_u32_f32 %0, %1", V1_V, F32CVT)                     \
  X(CVT, cvt_f16_f32, "v_cvt_f16_f32", "v_cvt_f16_f32 %0, %1", V1_V, F32H)                       \
  X(CVT, cvt_f32_f16, "v_cvt_f32_f16", "v_cvt_f32_f16 %0, %1", V1_V, F16)                        \
  X(CVT, cvt_pkrtz_f16_f32, "v_cvt_pkrtz_f16_f32", "v_cvt_pkrtz_f16_f32 %0, %1, %2", V1_VV, F32H) \
  X(CVT, cvt_pk_bf16_f32, "v_cvt_pk_bf16_f32", "v_cvt_pk_bf16_f32 %0, %1, %2", V1_VV, F32)       \
  X(CVT, cvt_f64_f32, "v_cvt_f64_f32", "v_cvt_f64_f32 %0, %1", V2_V, F32)                        \
  X(CVT, cvt_f32_f64, "v_cvt_f32_f64", "v_cvt_f32_f64 %0, %1", V1_D, F64R)                       \
  X(CVT, cvt_f64_i32, "v_cvt_f64_i32", "v_cvt_f64_i32 %0, %1", V2_V, INT)                        \
  X(CVT, cvt_i32_f64, "v_cvt_i32_f64", "v_cvt_i32_f64 %0, %1", V1_D, F64R)                       \
  X(CVT, cvt_f32_ubyte0, "v_cvt_f32_ubyte0", "v_cvt_f32_ubyte0 %0, %1", V1_V, INT)               \
  X(CVT, cvt_f32_ubyte1, "v_cvt_f32_ubyte1", "v_cvt_f32_ubyte1 %0, %1", V1_V, INT)               \
  X(CVT, cvt_f32_ubyte2, "v_cvt_f32_ubyte2", "v_cvt_f32_ubyte2 %0, %1", V1_V, INT)               \
  X(CVT, cvt_f32_ubyte3, "v_cvt_f32_ubyte3", "v_cvt_f32_ubyte3 %0, %1", V1_V, INT)               \
  X(CVT, cvt_pk_i16_i32, "v_cvt_pk_i16_i32", "v_cvt_pk_i16_i32 %0, %1, %2", V1_VV, INT)          \
  X(CVT, cvt_pk_u16_u32, "v_cvt_pk_u16_u32", "v_cvt_pk_u16_u32 %0, %1, %2", V1_VV, INT)          \
  X(CVT, cvt_pk_u8_f32, "v_cvt_pk_u8_f32", "v_cvt_pk_u8_f32 %0, %1, %2, %3", V1_VVV, F32U8)      \
  X(CVT, cvt_pknorm_i16_f32, "v_cvt_pknorm_i16_f32", "v_cvt_pknorm_i16_f32 %0, %1, %2", V1_VV, F32NORM) \
  X(SCALE, sc_pk_f32_fp8, "v_cvt_scalef32_pk_f32_fp8", "v_cvt_scalef32_pk_f32_fp8 %0, %1, %2", V2_VV, FP8) \
  X(SCALE, sc_pk32_f32_fp6_x2, "v_cvt_scalef32_pk32_f32_fp6", "v_cvt_scalef32_pk32_f32_fp6 %0, %1, 2.0", V2_FP6, FP6) \
  X(SCALE, sc_pk32_f32_fp6_half, "v_cvt_scalef32_pk32_f32_fp6", "v_cvt_scalef32_pk32_f32_fp6 %0, %1, 0.5", V2_FP6, FP6) \
  X(SCALE, sc_pk_fp8_f16, "v_cvt_scalef32_pk_fp8_f16", "v_cvt_scalef32_pk_fp8_f16 %0, %1, %2", V1_VVO, SCALEF16) \
  X(SCALE, sc_pk_fp8_bf16, "v_cvt_scalef32_pk_fp8_bf16", "v_cvt_scalef32_pk_fp8_bf16 %0, %1, %2", V1_VVO, SCALEBF16) \
  X(SCALE, sc_pk_f32_fp8_hi, "v_cvt_scalef32_pk_f32_fp8", "v_cvt_scalef32_pk_f32_fp8 %0, %1, %2 op_sel:[1,0,0]", V2_VV, FP8) \
  X(SCALE, sc_pk_f32_bf8, "v_cvt_scalef32_pk_f32_bf8", "v_cvt_scalef32_pk_f32_bf8 %0, %1, %2", V2_VV, BF8) \
  X(SCALE, sc_pk_f32_fp4, "v_cvt_scalef32_pk_f32_fp4", "v_cvt_scalef32_pk_f32_fp4 %0, %1, %2", V2_VV, FP4) \
  X(SCALE, sc_pk_fp8_f32, "v_cvt_scalef32_pk_fp8_f32", "v_cvt_scalef32_pk_fp8_f32 %0, %1, %2, %3", V1_VVVO, SCALEF32) \
  X(SCALE, sc_pk_fp8_f32_hi, "v_cvt_scalef32_pk_fp8_f32", "v_cvt_scalef32_pk_fp8_f32 %0, %1, %2, %3 op_sel:[0,0,0,1]", V1_VVVO, SCALEF32) \
  X(SCALE, sc_pk_bf8_f32, "v_cvt_scalef32_pk_bf8_f32", "v_cvt_scalef32_pk_bf8_f32 %0, %1, %2, %3", V1_VVVO, SCALEF32) \
  X(SCALE, sc_pk_fp4_f32, "v_cvt_scalef32_pk_fp4_f32", "v_cvt_scalef32_pk_fp4_f32 %0, %1, %2, %3", V1_VVVO, SCALEF32) \
  CRO_ALU_XCMPF(X, lt) CRO_ALU_XCMPF(X, le) CRO_ALU_XCMPF(X, eq) CRO_ALU_XCMPF(X, lg)             \
  CRO_ALU_XCMPF(X, gt) CRO_ALU_XCMPF(X, ge) CRO_ALU_XCMPF(X, o) CRO_ALU_XCMPF(X, u)               \
  CRO_ALU_XCMPF(X, nge) CRO_ALU_XCMPF(X, nlt)                                                     \
  CRO_ALU_XCMPD(X, lt) CRO_ALU_XCMPD(X, le) CRO_ALU_XCMPD(X, eq) CRO_ALU_XCMPD(X, lg)             \
  CRO_ALU_XCMPD(X, gt) CRO_ALU_XCMPD(X, ge)                                                       \
  CRO_ALU_XCMPH(X, lt) CRO_ALU_XCMPH(X, le) CRO_ALU_XCMPH(X, eq) CRO_ALU_XCMPH(X, lg)             \
  CRO_ALU_XCMPH(X, gt) CRO_ALU_XCMPH(X, ge)                                                       \
  CRO_ALU_XCMPI(X, lt) CRO_ALU_XCMPI(X, eq) CRO_ALU_XCMPI(X, gt) CRO_ALU_XCMPI(X, ne)             \
  X(CMP, cmp_class_f32, "v_cmp_class_f32", CMPT("v_cmp_class_f32"), V1_VV, CLASS32)              \
  X(CMP, cmp_class_f64, "v_cmp_class_f64", CMPT("v_cmp_class_f64"), V1_DV, CLASS64)              \
  X(CMP, cmpx_lt_u32, "v_cmpx_lt_u32", "s_mov_b64 %1, exec\n\tv_cmpx_lt_u32 vcc, %2, %3\n\tv_mov_b32 %0, %2\n\ts_mov_b64 exec, %1", V1_CMPX, INT) \
  X(SALU, s_add_u64, "s_addc_u32", "s_add_u32 %0, %2, %3\n\ts_addc_u32 %1, %4, %5", S2C_SSSS, INT) \
  X(SALU, s_sub_u64, "s_subb_u32", "s_sub_u32 %0, %2, %3\n\ts_subb_u32 %1, %4, %5", S2C_SSSS, INT) \
  CRO_ALU_XS2(X, s_mul_i32) CRO_ALU_XS2(X, s_mul_hi_u32) CRO_ALU_XS2(X, s_mul_hi_i32)             \
  CRO_ALU_XS2C(X, s_lshl_b32) CRO_ALU_XS2C(X, s_lshr_b32) CRO_ALU_XS2C(X, s_ashr_i32)             \
  X(SALU, s_lshl_b64, "s_lshl_b64", "s_lshl_b64 %0, %1, %2", S2_QS, INT)                         \
  X(SALU, s_lshr_b64, "s_lshr_b64", "s_lshr_b64 %0, %1, %2", S2_QS, INT)                         \
  X(SALU, s_ashr_i64, "s_ashr_i64", "s_ashr_i64 %0, %1, %2", S2_QS, INT)                         \
  CRO_ALU_XS2C(X, s_and_b32) CRO_ALU_XS2C(X, s_or_b32) CRO_ALU_XS2C(X, s_xor_b32)                 \
  CRO_ALU_XS2C(X, s_nand_b32) CRO_ALU_XS2C(X, s_nor_b32) CRO_ALU_XS2C(X, s_xnor_b32)              \
  CRO_ALU_XS2C(X, s_andn2_b32) CRO_ALU_XS2C(X, s_orn2_b32)                                        \
  CRO_ALU_XS64(X, s_and_b64) CRO_ALU_XS64(X, s_or_b64) CRO_ALU_XS64(X, s_xor_b64)                 \
  CRO_ALU_XS64(X, s_nand_b64) CRO_ALU_XS64(X, s_nor_b64) CRO_ALU_XS64(X, s_xnor_b64)              \
  CRO_ALU_XS64(X, s_andn2_b64) CRO_ALU_XS64(X, s_orn2_b64)                                        \
  X(SALU, s_not_b32, "s_not_b32", "s_not_b32 %0, %2\n\ts_cselect_b32 %1, 1, 0", S1C_S, INT)      \
  X(SALU, s_brev_b32, "s_brev_b32", "s_brev_b32 %0, %1", S1_S, INT)                              \
  X(SALU, s_brev_b64, "s_brev_b64", "s_brev_b64 %0, %1", S2_Q, INT)                              \
  X(SALU, s_bcnt0_i32_b32, "s_bcnt0_i32_b32", "s_bcnt0_i32_b32 %0, %2\n\ts_cselect_b32 %1, 1, 0", S1C_S, INT) \
  X(SALU, s_bcnt1_i32_b64, "s_bcnt1_i32_b64", "s_bcnt1_i32_b64 %0, %2\n\ts_cselect_b32 %1, 1, 0", S1C_Q, INT) \
  X(SALU, s_ff0_i32_b32, "s_ff0_i32_b32", "s_ff0_i32_b32 %0, %1", S1_S, INT)                     \
  X(SALU, s_ff1_i32_b32, "s_ff1_i32_b32", "s_ff1_i32_b32 %0, %1", S1_S, INT)                     \
  X(SALU, s_ff1_i32_b64, "s_ff1_i32_b64", "s_ff1_i32_b64 %0, %1", S1_Q, INT)                     \
  X(SALU, s_flbit_i32_b32, "s_flbit_i32_b32", "s_flbit_i32_b32 %0, %1", S1_S, INT)               \
  X(SALU, s_flbit_i32, "s_flbit_i32", "s_flbit_i32 %0, %1", S1_S, INT)                           \
  X(SALU, s_flbit_i32_b64, "s_flbit_i32_b64", "s_flbit_i32_b64 %0, %1", S1_Q, INT)               \
  X(SALU, s_sext_i32_i8, "s_sext_i32_i8", "s_sext_i32_i8 %0, %1", S1_S, INT)                     \
  X(SALU, s_sext_i32_i16, "s_sext_i32_i16", "s_sext_i32_i16 %0, %1", S1_S, INT)                  \
  CRO_ALU_XS2(X, s_bfm_b32) CRO_ALU_XS2C(X, s_bfe_u32) CRO_ALU_XS2C(X, s_bfe_i32)                 \
  X(SALU, s_bfe_u64, "s_bfe_u64", "s_bfe_u64 %0, %1, %2", S2_QS, INT)                            \
  X(SALU, s_bfe_i64, "s_bfe_i64", "s_bfe_i64 %0, %1, %2", S2_QS, INT)                            \
  CRO_ALU_XSCQ(X, s_and_b64, SC_QQ) CRO_ALU_XSCQ(X, s_or_b64, SC_QQ) CRO_ALU_XSCQ(X, s_xor_b64, SC_QQ) \
  CRO_ALU_XSCQ(X, s_nand_b64, SC_QQ) CRO_ALU_XSCQ(X, s_nor_b64, SC_QQ) CRO_ALU_XSCQ(X, s_xnor_b64, SC_QQ) \
  CRO_ALU_XSCQ(X, s_andn2_b64, SC_QQ) CRO_ALU_XSCQ(X, s_orn2_b64, SC_QQ)                          \
  CRO_ALU_XSCQ(X, s_lshl_b64, SC_QS) CRO_ALU_XSCQ(X, s_lshr_b64, SC_QS) CRO_ALU_XSCQ(X, s_ashr_i64, SC_QS) \
  CRO_ALU_XSCQ(X, s_bfe_u64, SC_QS) CRO_ALU_XSCQ(X, s_bfe_i64, SC_QS)                             \
  X(SALU, s_add_u64_scc, "s_addc_u32", "s_add_u32 %1, %3, %4\n\ts_addc_u32 %2, %5, %6\n\ts_cselect_b32 %0, 1, 0", SC_SSSS, INT) \
  X(SALU, s_sub_u64_scc, "s_subb_u32", "s_sub_u32 %1, %3, %4\n\ts_subb_u32 %2, %5, %6\n\ts_cselect_b32 %0, 1, 0", SC_SSSS, INT) \
  CRO_ALU_XSEL(X, eq, i32) CRO_ALU_XSEL(X, lg, i32) CRO_ALU_XSEL(X, lt, i32)                      \
  CRO_ALU_XSEL(X, gt, i32) CRO_ALU_XSEL(X, eq, u32) CRO_ALU_XSEL(X, lg, u32)                      \
  CRO_ALU_XSEL(X, lt, u32) CRO_ALU_XSEL(X, gt, u32)                                               \
  CRO_ALU_XS2C(X, s_absdiff_i32) CRO_ALU_XS2C(X, s_min_i32) CRO_ALU_XS2C(X, s_max_u32)            \
  CRO_ALU_XS2C(X, s_lshl1_add_u32) CRO_ALU_XS2C(X, s_lshl2_add_u32)                               \
  CRO_ALU_XS2C(X, s_lshl3_add_u32) CRO_ALU_XS2C(X, s_lshl4_add_u32)                               \
  CRO_ALU_XS2(X, s_pack_ll_b32_b16) CRO_ALU_XS2(X, s_pack_lh_b32_b16)                             \
  CRO_ALU_XS2(X, s_pack_hh_b32_b16)                                                               \
  CRO_ALU_XT(X, exp_f32, V1_V, TEXP) CRO_ALU_XT(X, log_f32, V1_V, TLOG)                           \
  CRO_ALU_XT(X, rcp_f32, V1_V, TRCP) CRO_ALU_XT(X, rsq_f32, V1_V, TSQRT)                          \
  CRO_ALU_XT(X, sqrt_f32, V1_V, TSQRT) CRO_ALU_XT(X, sin_f32, V1_V, TSIN)                         \
  CRO_ALU_XT(X, cos_f32, V1_V, TSIN) CRO_ALU_XT(X, rcp_f64, V2_D, TRCP64)                         \
  CRO_ALU_XT(X, rsq_f64, V2_D, TSQRT64) CRO_ALU_XT(X, sqrt_f64, V2_D, TSQRT64)                    \
  CRO_ALU_XT(X, exp_f16, V1_V, TEXP16) CRO_ALU_XT(X, log_f16, V1_V, TLOG16)                       \
  CRO_ALU_XT(X, rcp_f16, V1_V, TRCP16) CRO_ALU_XT(X, sqrt_f16, V1_V, TSQRT16)

enum {
#define CRO_ALU_X(check, name, mnem, tmpl, sig, cls) CRO_ALU_FORM_##name,
  CRO_ALU_FORMS(CRO_ALU_X)
#undef CRO_ALU_X
      CRO_ALU_FORM_COUNT
};

struct CroAluForm {
  int check;
  const char* name;
  const char* mnemonic;
  int sig, nsrc, nres, cls;
  void (*ref)(const uint32_t* s, uint32_t* w);
};

static inline const CroAluForm* cro_alu_form(int form) {
  static const CroAluForm forms[CRO_ALU_FORM_COUNT] = {
#define CRO_ALU_X(check, name, mnem, tmpl, sig, cls)                                  \
  {CRO_ALU_##check, #name, mnem, CRO_ALU_SIG_##sig, CRO_ALU_NSRC_##sig, CRO_ALU_NRES_##sig, \
   CRO_ALU_C_##cls, cro_alu_r_##name},
      CRO_ALU_FORMS(CRO_ALU_X)
#undef CRO_ALU_X
  };
  return form < 0 || form >= CRO_ALU_FORM_COUNT ? nullptr : &forms[form];
}

// Rows of a form whose result words are compared with the table: all, of a
// transcendental form its anchors.  v_sqrt_f64 has none: it is an
// approximation that misses even powers of four by bit 26 of the low word.
CRO_COV_HD static inline constexpr int cro_alu_checked_rows(int check, int form) {
  return check != CRO_ALU_TRANS ? (int)CRO_ALU_ROWS
         : form == CRO_ALU_FORM_t_sqrt_f64 ? 0 : (int)CRO_ALU_ANCHORS;
}

CRO_COV_HD static inline uint32_t cro_alu_elem(int form, int word, int row, int lane) {
  return ((uint32_t)form << 13) | ((uint32_t)word << 12) | ((uint32_t)row << 6) | (uint32_t)lane;
}

// -- operand rows ----------------------------------------------------------------------

enum { CRO_ALU_INT_EDGES = 15, CRO_ALU_F32_EDGES = 14, CRO_ALU_F64_EDGES = 10 };

// 0, 1, all ones, the sign bit, carries out of bits 15, 23 and 31 (of s0 + s1
// and of the 64-bit s1:s0 + s3:s2), shift counts 0, 31, 32 and 63 as the
// first and as the second operand
static const uint32_t kCroAluIntEdges[CRO_ALU_INT_EDGES][6] = {
    {0, 0, 0, 0, 0, 0},
    {1, 1, 1, 1, 1, 1},
    {~0u, ~0u, ~0u, ~0u, ~0u, ~0u},
    {0x80000000u, 0x80000000u, 0x80000000u, 0x80000000u, 1, 0},
    {0x0000FFFFu, 1, 0x0000FFFFu, 0, 1, 0},
    {0x00FFFFFFu, 1, 0x00FFFFFFu, 0, 1, 0},
    {0xFFFFFFFFu, 1, 0xFFFFFFFFu, 0, 1, 0},
    {0, 0x12345678u, 0x9ABCDEF0u, 0, 0x0F0F0F0Fu, 0},
    {31, 0x12345678u, 0x9ABCDEF0u, 31, 0x0F0F0F0Fu, 31},
    {32, 0x12345678u, 0x9ABCDEF0u, 32, 0x0F0F0F0Fu, 32},
    {63, 0x12345678u, 0x9ABCDEF0u, 63, 0x0F0F0F0Fu, 63},
    {0x92345678u, 0, 0, 0x9ABCDEF0u, 0, 0},
    {0x92345678u, 31, 31, 0x9ABCDEF0u, 31, 31},
    {0x92345678u, 32, 32, 0x9ABCDEF0u, 32, 32},
    {0x92345678u, 63, 63, 0x9ABCDEF0u, 63, 63},
};

// +-0, smallest and largest normal and subnormal, ties to even in both
// directions (1 + 2^-24 down, 1 + 2^-23 + 2^-24 up), overflow to infinity
// (by doubling, and by a tie at the largest normal)
static const uint32_t kCroAluF32Edges[CRO_ALU_F32_EDGES][3] = {
    {0x00000000u, 0x80000000u, 0x00000000u}, {0x80000000u, 0x80000000u, 0x00000000u},
    {0x00800000u, 0x00800000u, 0x80800000u}, {0x7F7FFFFFu, 0x7F7FFFFFu, 0x7F7FFFFFu},
    {0x00000001u, 0x00000001u, 0x80000001u}, {0x007FFFFFu, 0x00000001u, 0x807FFFFFu},
    {0x3F800000u, 0x33800000u, 0x00000000u}, {0x3F800001u, 0x33800000u, 0x80000000u},
    {0x7F7FFFFFu, 0x73000000u, 0x3F800000u}, {0xFF7FFFFFu, 0xFF7FFFFFu, 0x3F800000u},
    {0x3F801000u, 0x3F801000u, 0x3F800000u}, {0x00800000u, 0x3F000000u, 0x00000001u},
    {0xBFC00000u, 0x40200000u, 0x3F000000u}, {0x807FFFFFu, 0x00800000u, 0x3FC00000u},
};

// the fma classes' own edge rows (within the bound): ties in both
// directions, subnormal results, overflow by a tie, zeros
static const uint32_t kCroAluFmaEdges[8][3] = {
    {0x3F800000u, 0x3F800000u, 0x33800000u}, {0x3F800001u, 0x3F800000u, 0x33800000u},
    {0x00000000u, 0x80000000u, 0x00000000u}, {0x00800000u, 0x3F800000u, 0x00000001u},
    {0x007FFFFFu, 0x3F800000u, 0x80000001u}, {0x7F7FFFFFu, 0x3F800000u, 0x73000000u},
    {0x3F801000u, 0x3F801000u, 0xB3800000u}, {0x1E000000u, 0x1E000000u, 0x00000003u},
};

static inline uint32_t cro_alu_f32_bits(uint32_t x, int e_lo, int e_n) {  // 2^e_lo .. 2^(e_lo+e_n)
  return (x & 0x80000000u) | ((uint32_t)(127 + e_lo + (int)((x >> 23) & 255u) % e_n) << 23) | (x & 0x7FFFFFu);
}
static inline uint32_t cro_alu_f16_bits(uint32_t x, int e_lo, int e_n) {
  return (x & 0x8000u) | ((uint32_t)(15 + e_lo + (int)((x >> 10) & 31u) % e_n) << 10) | (x & 0x3FFu);
}
// an (a, b, c) triple of f32 within the fma bound
static inline void cro_alu_fma_triple(uint32_t x, uint32_t y, uint32_t z, uint32_t* a, uint32_t* b, uint32_t* c) {
  *a = cro_alu_f32_bits(x, -8, 17);
  *b = cro_alu_f32_bits(y, -8, 17);
  const int eab = (int)((*a >> 23) & 255u) + (int)((*b >> 23) & 255u) - 254;
  *c = (z & 0x807FFFFFu) | ((uint32_t)(127 + eab + (int)((z >> 23) & 255u) % 9 - 4) << 23);
}
static inline uint32_t cro_alu_f16_fma_c(uint32_t a, uint32_t b, uint32_t z) {
  int ec = (int)((a >> 10) & 31u) + (int)((b >> 10) & 31u) - 30 + (int)((z >> 10) & 31u) % 9 - 4;
  ec = ec < -14 ? -14 : ec > 15 ? 15 : ec;
  return (z & 0x83FFu) | ((uint32_t)(ec + 15) << 10);
}
// a 21-bit odd integer times 2^e, e in e_lo .. e_lo + e_n - 1
static inline uint64_t cro_alu_f64_small(uint32_t x, int e_lo, int e_n) {
  const double v = ldexp((double)((x & 0x1FFFFFu) | 0x100001u), e_lo + (int)((x >> 21) & 255u) % e_n - 20);
  return cro_alu_ud((x >> 31) ? -v : v);
}
static inline uint64_t cro_alu_f64_full(uint32_t x, uint32_t y, int e_lo, int e_n) {
  return ((uint64_t)(x & 0x80000000u) << 32) | ((uint64_t)(1023 + e_lo + (int)((x >> 20) & 2047u) % e_n) << 52) |
         ((uint64_t)(x & 0xFFFFFu) << 32) | y;
}

static const uint64_t kCroAluF64Edges[CRO_ALU_F64_EDGES][2] = {
    {0x0000000000000000ull, 0x8000000000000000ull}, {0x0010000000000000ull, 0x0010000000000000ull},
    {0x7FEFFFFFFFFFFFFFull, 0x7FEFFFFFFFFFFFFFull}, {0x0000000000000001ull, 0x0000000000000001ull},
    {0x000FFFFFFFFFFFFFull, 0x8000000000000001ull}, {0x3FF0000000000000ull, 0x3CA0000000000000ull},
    {0x3FF0000000000001ull, 0x3CA0000000000000ull}, {0x7FEFFFFFFFFFFFFFull, 0x7C90000000000000ull},
    // the divide's scale path: a tiny divisor, a huge quotient
    {0x3FF8000000000000ull, 0x0000000000000003ull}, {0x7E37E43C8800759Cull, 0x3EB0000000000000ull},
};

// the f64 fma's own edge rows, results exact or one IEEE rounding of a sum
// both sides form the same way: +-0, subnormal operand and result, smallest
// and largest normal, a tie (1 * 1 + 2^-53), overflow to infinity
enum { CRO_ALU_F64FMA_EDGES = 7 };
static const uint64_t kCroAluF64FmaEdges[CRO_ALU_F64FMA_EDGES][3] = {
    {0x0000000000000000ull, 0x8000000000000000ull, 0x0000000000000000ull},
    {0x0000000000000001ull, 0x3FF0000000000000ull, 0x8000000000000003ull},
    {0x0010000000000000ull, 0x3FF0000000000000ull, 0x0000000000000001ull},
    {0x7FEFFFFFFFFFFFFFull, 0x3FF0000000000000ull, 0x0000000000000000ull},
    {0x3FF0000000000000ull, 0x3FF0000000000000ull, 0x3CA0000000000000ull},
    {0x3FF0000000000001ull, 0x3FF0000000000000ull, 0x3CA0000000000000ull},
    {0x7FE0000000000000ull, 0x4000000000000000ull, 0x7FE0000000000000ull},
};

static const uint32_t kCroAluCmpF32[12] = {0x7FC00000u, 0x00000000u, 0x80000000u, 0x3F800000u,
                                           0xBF800000u, 0x3F800001u, 0x7F800000u, 0xFF800000u,
                                           0x00000001u, 0x80000001u, 0x7F800001u, 0x42280000u};
static const uint32_t kCroAluCmpF16[8] = {0x0000u, 0x8000u, 0x3C00u, 0xBC00u, 0x3C01u, 0x0001u, 0x8001u, 0x7BFFu};
static const uint64_t kCroAluCmpF64[8] = {0x0000000000000000ull, 0x8000000000000000ull, 0x3FF0000000000000ull,
                                          0xBFF0000000000000ull, 0x3FF0000000000001ull, 0x0000000000000001ull,
                                          0x8000000000000001ull, 0x7FEFFFFFFFFFFFFFull};
// one value of each class, in class-bit order
static const uint32_t kCroAluClassF32[10] = {0x7F800001u, 0x7FC00000u, 0xFF800000u, 0xC0490FDBu, 0x80000400u,
                                             0x80000000u, 0x00000000u, 0x00000400u, 0x40490FDBu, 0x7F800000u};
static const uint64_t kCroAluClassF64[10] = {
    0x7FF0000000000001ull, 0x7FF8000000000000ull, 0xFFF0000000000000ull, 0xC00921FB54442D18ull,
    0x8000000000000400ull, 0x8000000000000000ull, 0x0000000000000000ull, 0x0000000000000400ull,
    0x400921FB54442D18ull, 0x7FF0000000000000ull};

// the six source words of row `row` of form `form`
static inline void cro_alu_sources(uint32_t seed, int form, int row, uint32_t* s) {
  const CroAluForm* fm = cro_alu_form(form);
  uint32_t x[6];
  for (int k = 0; k < 6; ++k) x[k] = cro_alu_rand(seed, form, row, k);
  const float scale = (float)ldexp(1.0, (int)(x[5] % 9u) - 4);
  switch (fm->cls) {
    case CRO_ALU_C_INT:
      for (int k = 0; k < 6; ++k) s[k] = row < CRO_ALU_INT_EDGES ? kCroAluIntEdges[row][k] : x[k];
      break;
    case CRO_ALU_C_PERM:
      for (int k = 0; k < 6; ++k) s[k] = x[k];
      s[2] = row < 4 ? 0x03020100u + 0x04040404u * (uint32_t)row : x[2] & 0x0F0F0F0Fu;
      break;
    case CRO_ALU_C_F32:
      for (int k = 0; k < 6; ++k)
        s[k] = row < CRO_ALU_F32_EDGES ? kCroAluF32Edges[row][k % 3] : cro_alu_f32_bits(x[k], -7, 34);
      break;
    case CRO_ALU_C_F32FMA:
    case CRO_ALU_C_F32PKFMA: {
      uint32_t t[6];
      for (int p = 0; p < 2; ++p) {
        if (row < 8) for (int k = 0; k < 3; ++k) t[3 * p + k] = kCroAluFmaEdges[(row + p) % 8][k];
        else cro_alu_fma_triple(x[3 * p], x[3 * p + 1], x[3 * p + 2], &t[3 * p], &t[3 * p + 1], &t[3 * p + 2]);
      }
      for (int k = 0; k < 6; ++k) s[k] = fm->cls == CRO_ALU_C_F32FMA ? t[k] : t[3 * (k & 1) + (k >> 1)];
      break;
    }
    case CRO_ALU_C_F32I: {
      static const uint32_t edges[6][2] = {{0x00000001u, 10}, {0x7F7FFFFFu, 1}, {0x3F800000u, (uint32_t)-149},
                                           {0x3F800000u, (uint32_t)-150}, {0x40400000u, (uint32_t)-150}, {0x80000000u, 5}};
      s[0] = row < 6 ? edges[row][0] : cro_alu_f32_bits(x[0], -20, 41);
      s[1] = row < 6 ? edges[row][1] : (uint32_t)((int)(x[1] % 81u) - 40);
      for (int k = 2; k < 6; ++k) s[k] = x[k];
      break;
    }
    case CRO_ALU_C_F32U8: {
      // ties in both directions, both clamps, -0; else values around 0..512
      static const uint32_t edges[10] = {0x3F000000u, 0x3FC00000u, 0x40200000u, 0x437F8000u, 0x43800000u,
                                         0xBF800000u, 0x437E8000u, 0x80000000u, 0x00000001u, 0x437F0000u};
      s[0] = row < 10 ? edges[row] : cro_alu_f32_bits(x[0], -3, 12);
      s[1] = row < 10 ? (uint32_t)row : x[1];
      for (int k = 2; k < 6; ++k) s[k] = x[k];
      break;
    }
    case CRO_ALU_C_F32NORM: {
      static const uint32_t edges[8] = {0x3F800000u, 0xBF800000u, 0x40000000u, 0xC0000000u,
                                        0x00000000u, 0x80000000u, 0x3F000000u, 0x37800100u};
      for (int k = 0; k < 6; ++k) s[k] = row < 8 ? edges[(row + k) % 8] : cro_alu_f32_bits(x[k], -18, 19);
      break;
    }
    case CRO_ALU_C_SCALEF16:
    case CRO_ALU_C_SCALEBF16: {
      // saturating values, a tie between codes, zeros; else across e4m3's range
      static const int edges[4][2] = {{30000, -30000}, {464, 480}, {0, 0}, {17, 19}};
      for (int h = 0; h < 2; ++h) {
        const double v = row < 4 ? (double)edges[row][h] / (row == 3 ? 16.0 : 1.0)
                                 : (double)cro_alu_f(cro_alu_f32_bits(x[h], -9, 19) & 0xFFFF0000u);
        const uint32_t bits = fm->cls == CRO_ALU_C_SCALEF16 ? cro_alu_h_of(v) : cro_alu_u((float)v) >> 16;
        s[0] = h ? s[0] | (bits << 16) : bits;
      }
      if (row == 2) s[0] = 0x80000000u;
      s[1] = cro_alu_u(row < 4 ? 1.0f : scale);
      for (int k = 2; k < 6; ++k) s[k] = x[k];
      break;
    }
    case CRO_ALU_C_F32CVT: {
      static const uint32_t edges[12] = {0x7FC00000u, 0x7F800000u, 0xFF800000u, 0x4F000000u, 0xCF000000u, 0x4F800000u,
                                         0x4EFFFFFFu, 0xBF800000u, 0x3F7FFFFFu, 0x00000000u, 0x80000000u, 0xCF000001u};
      for (int k = 0; k < 6; ++k) s[k] = row < 12 ? edges[(row + k) % 12] : cro_alu_f32_bits(x[k], -2, 36);
      break;
    }
    case CRO_ALU_C_F32H: {
      // ties at the half's precision in both directions, its overflow
      // threshold, its subnormal range
      static const uint32_t edges[10] = {0x3F801000u, 0x3F803000u, 0x477FF000u, 0x477FEFFFu, 0x33000000u,
                                         0x33800000u, 0x33C00000u, 0x38800000u, 0x80000000u, 0x387FC000u};
      for (int k = 0; k < 6; ++k) s[k] = row < 10 ? edges[(row + k) % 10] : cro_alu_f32_bits(x[k], -26, 43);
      break;
    }
    case CRO_ALU_C_F16: {
      static const uint32_t edges[8][2] = {{0x80000000u, 0x00008000u}, {0x04000400u, 0x04000400u}, {0x7BFF7BFFu, 0x7BFF7BFFu},
                                           {0x00010001u, 0x00018001u}, {0x03FF03FFu, 0x00018001u}, {0x3C003C01u, 0x10001000u},
                                           {0x7BFF7BFFu, 0x5000D000u}, {0x3C013C01u, 0x3C013C01u}};
      for (int k = 0; k < 6; ++k)
        s[k] = row < 8 ? edges[row][k & 1]
                       : cro_alu_f16_bits(x[k], -10, 20) | (cro_alu_f16_bits(x[k] >> 16, -10, 20) << 16);
      break;
    }
    case CRO_ALU_C_F16FMA:
      for (int k = 0; k < 6; ++k) s[k] = x[k];
      for (int h = 0; h < 32; h += 16) {
        const uint32_t ha = cro_alu_f16_bits(x[0] >> h, -6, 13), hb = cro_alu_f16_bits(x[1] >> h, -6, 13);
        const uint32_t hc = cro_alu_f16_fma_c(ha, hb, x[2] >> h);
        const uint32_t m = 0xFFFFu << h;
        s[0] = (s[0] & ~m) | (ha << h);
        s[1] = (s[1] & ~m) | (hb << h);
        s[2] = (s[2] & ~m) | (hc << h);
      }
      {
        // ties in both directions, +-0, subnormal operands and results, the
        // largest normal, overflow by a tie: (a, b, c) per half, in bound
        static const uint32_t edges[6][3] = {{0x3C003C00u, 0x3C013C00u, 0x10001000u}, {0x00008000u, 0x3C003C00u, 0x80000000u},
                                             {0x00010001u, 0x3C003C00u, 0x800103FFu}, {0x04003800u, 0x38000001u, 0x00010001u},
                                             {0x7BFF7BFFu, 0x3C003C00u, 0x4C004BFFu}, {0x7BFFFBFFu, 0x3C00BC00u, 0x00000000u}};
        if (row < 6) { s[0] = edges[row][0]; s[1] = edges[row][1]; s[2] = edges[row][2]; }
      }
      break;
    case CRO_ALU_C_F64:
    case CRO_ALU_C_F64FMA:
      if (row < CRO_ALU_F64_EDGES && fm->cls == CRO_ALU_C_F64) {
        cro_alu_w64(s, kCroAluF64Edges[row][0]);
        cro_alu_w64(s + 2, kCroAluF64Edges[row][1]);
        cro_alu_w64(s + 4, kCroAluF64Edges[row][0]);
      } else if (row < CRO_ALU_F64FMA_EDGES) {
        for (int k = 0; k < 3; ++k) cro_alu_w64(s + 2 * k, kCroAluF64FmaEdges[row][k]);
      } else {
        const uint64_t va = cro_alu_f64_small(x[0], -4, 9), vb = cro_alu_f64_small(x[1], -4, 9);
        cro_alu_w64(s, va);
        cro_alu_w64(s + 2, vb);
        // c: within 2^-6 .. 2^6 of the product's exponent
        const int eab = (int)((va >> 52) & 2047u) + (int)((vb >> 52) & 2047u) - 2046;
        cro_alu_w64(s + 4, fm->cls == CRO_ALU_C_F64 ? cro_alu_f64_small(x[2], -4, 9)
                                                    : cro_alu_f64_small(x[2], eab - 6, 13));
      }
      break;
    case CRO_ALU_C_F64DIV:
      if (row < CRO_ALU_F64_EDGES - 1) {
        cro_alu_w64(s, kCroAluF64Edges[row + 1][0]);
        cro_alu_w64(s + 2, kCroAluF64Edges[row + 1][1]);
      } else {
        cro_alu_w64(s, cro_alu_f64_full(x[0], x[1], -3, 58));
        cro_alu_w64(s + 2, cro_alu_f64_full(x[2], x[3], -3, 58));
      }
      s[1] &= 0x7FFFFFFFu;
      s[4] = x[4]; s[5] = x[5];
      break;
    case CRO_ALU_C_F64R:
    case CRO_ALU_C_F64I:
      if (row < CRO_ALU_F64_EDGES) {
        cro_alu_w64(s, kCroAluF64Edges[row][0]);
        cro_alu_w64(s + 2, kCroAluF64Edges[row][1]);
      } else {
        cro_alu_w64(s, cro_alu_f64_full(x[0], x[1], -3, 58));
        cro_alu_w64(s + 2, cro_alu_f64_full(x[2], x[3], -3, 58));
      }
      s[4] = x[4]; s[5] = x[5];
      if (row >= 14 && row < 22) s[1] &= 0x7FFFFFFFu;  // positive: the square root's domain
      if (row >= 22 && row < 26) cro_alu_wd(s, (double)(int32_t)x[0] + 0.5);  // ties of rndne
      if (fm->cls == CRO_ALU_C_F64I) s[2] = (uint32_t)((int)(x[2] % 121u) - 60);
      break;
    case CRO_ALU_C_DOTF16:
    case CRO_ALU_C_DOTBF16:
      for (int k = 0; k < 2; ++k) {
        const int lo = (int)(x[k] % 33u) - 16, hi = (int)((x[k] >> 8) % 33u) - 16;
        s[k] = fm->cls == CRO_ALU_C_DOTF16
                   ? cro_alu_h_of((double)lo) | (cro_alu_h_of((double)hi) << 16)
                   : (cro_alu_u((float)lo) >> 16) | (cro_alu_u((float)hi) & 0xFFFF0000u);
      }
      s[2] = cro_alu_u((float)((int)(x[2] % 2001u) - 1000));
      s[3] = x[3]; s[4] = x[4]; s[5] = x[5];
      break;
    case CRO_ALU_C_FP8:
    case CRO_ALU_C_BF8:
    case CRO_ALU_C_FP4:
      s[0] = x[0];
      for (int k = 0; k < 32; k += 8) {  // no NaN or infinity codes
        const uint32_t code = (x[0] >> k) & 255u;
        if (fm->cls == CRO_ALU_C_FP8 && (code & 0x7Fu) == 0x7Fu) s[0] ^= 1u << k;
        if (fm->cls == CRO_ALU_C_BF8 && (code & 0x7Cu) == 0x7Cu) s[0] ^= 0x40u << k;
      }
      s[1] = cro_alu_u(scale);
      for (int k = 2; k < 6; ++k) s[k] = x[k];
      break;
    case CRO_ALU_C_FP6:
      for (int k = 0; k < 6; ++k) s[k] = row == 0 ? 0u : row == 1 ? ~0u : x[k];
      break;
    case CRO_ALU_C_SCALEF32: {
      // saturating rows, ties between codes, zero; else values across the formats' ranges
      static const uint32_t edges[6][2] = {{0x47000000u, 0xC7000000u}, {0x43E00000u, 0x43F00000u}, {0x3F880000u, 0x3F980000u},
                                           {0x00000000u, 0x80000000u}, {0x3FA00000u, 0x40200000u}, {0x3A800000u, 0x3B400000u}};
      s[0] = row < 6 ? edges[row][0] : cro_alu_f32_bits(x[0], -12, 24);
      s[1] = row < 6 ? edges[row][1] : cro_alu_f32_bits(x[1], -12, 24);
      s[2] = cro_alu_u(row < 6 ? 1.0f : scale);
      s[3] = x[3]; s[4] = x[4]; s[5] = x[5];
      break;
    }
    case CRO_ALU_C_CMPF32:
      s[0] = kCroAluCmpF32[x[0] % 12u]; s[1] = kCroAluCmpF32[x[1] % 12u];
      if (row < 12) { s[0] = kCroAluCmpF32[row]; s[1] = kCroAluCmpF32[(row * 5 + 1) % 12]; }
      for (int k = 2; k < 6; ++k) s[k] = x[k];
      break;
    case CRO_ALU_C_CMPF16:
      s[0] = kCroAluCmpF16[x[0] % 8u] | (x[0] & 0xFFFF0000u); s[1] = kCroAluCmpF16[x[1] % 8u] | (x[1] & 0xFFFF0000u);
      for (int k = 2; k < 6; ++k) s[k] = x[k];
      break;
    case CRO_ALU_C_CMPF64:
      cro_alu_w64(s, kCroAluCmpF64[x[0] % 8u]);
      cro_alu_w64(s + 2, kCroAluCmpF64[x[1] % 8u]);
      s[4] = x[4]; s[5] = x[5];
      break;
    case CRO_ALU_C_CMPINT: {
      static const uint32_t pool[4] = {0, 1, 0x80000000u, ~0u};
      s[0] = pool[x[0] & 3u]; s[1] = pool[(x[0] >> 2) & 3u];
      s[2] = pool[x[1] & 3u]; s[3] = pool[(x[1] >> 2) & 3u];
      if (x[2] & 1u) { s[2] = s[0]; if (x[2] & 2u) s[3] = s[1]; }
      if (row >= 32) { s[0] = x[0]; s[1] = x[3]; if (!(x[2] & 1u)) { s[2] = x[4]; s[3] = x[5]; } else s[2] = s[0]; }
      s[4] = x[4]; s[5] = x[5];
      break;
    }
    case CRO_ALU_C_CLASS32:
      s[0] = kCroAluClassF32[x[0] % 10u];
      s[1] = row < 10 ? 1u << row : x[1] & 0x3FFu;
      if (row < 20) s[0] = kCroAluClassF32[row % 10];
      for (int k = 2; k < 6; ++k) s[k] = x[k];
      break;
    case CRO_ALU_C_CLASS64:
      cro_alu_w64(s, kCroAluClassF64[row < 20 ? (uint32_t)row % 10u : x[0] % 10u]);
      s[2] = row < 10 ? 1u << row : x[1] & 0x3FFu;
      s[3] = x[3]; s[4] = x[4]; s[5] = x[5];
      break;
    default: {
      // transcendental: anchors in the first rows, then normal inputs whose
      // results stay normal
      const int k = row - 8;  // anchors: -8 .. 7
      const bool anchor = row < CRO_ALU_ANCHORS;
      double v;
      switch (fm->cls) {
        case CRO_ALU_C_TEXP: v = anchor ? (double)k : (double)cro_alu_f(cro_alu_f32_bits(x[0], -6, 12)); break;
        case CRO_ALU_C_TLOG: v = anchor ? ldexp(1.0, 3 * k) : fabs((double)cro_alu_f(cro_alu_f32_bits(x[0], -60, 120))); break;
        case CRO_ALU_C_TRCP: v = anchor ? ldexp(k & 1 ? -1.0 : 1.0, 5 * k) : (double)cro_alu_f(cro_alu_f32_bits(x[0], -60, 120)); break;
        case CRO_ALU_C_TSQRT: v = anchor ? ldexp(1.0, 6 * k) : fabs((double)cro_alu_f(cro_alu_f32_bits(x[0], -60, 120))); break;
        case CRO_ALU_C_TSIN: v = anchor ? 0.25 * (double)k : (double)cro_alu_f(cro_alu_f32_bits(x[0], -6, 12)); break;
        case CRO_ALU_C_TRCP64: v = anchor ? ldexp(k & 1 ? -1.0 : 1.0, 37 * k) : cro_alu_d(x[1], (uint32_t)(cro_alu_f64_full(x[0], 0, -300, 600) >> 32)); break;
        case CRO_ALU_C_TSQRT64: v = anchor ? ldexp(1.0, 38 * k) : fabs(cro_alu_d(x[1], (uint32_t)(cro_alu_f64_full(x[0], 0, -300, 600) >> 32))); break;
        case CRO_ALU_C_TEXP16: v = anchor ? (double)k : cro_alu_h(cro_alu_f16_bits(x[0], -4, 7)); break;
        case CRO_ALU_C_TLOG16: v = anchor ? ldexp(1.0, k) : fabs(cro_alu_h(cro_alu_f16_bits(x[0], -10, 20))); break;
        case CRO_ALU_C_TRCP16: v = anchor ? ldexp(k & 1 ? -1.0 : 1.0, k) : cro_alu_h(cro_alu_f16_bits(x[0], -10, 20)); break;
        default: v = anchor ? ldexp(1.0, 2 * (k / 2)) : fabs(cro_alu_h(cro_alu_f16_bits(x[0], -10, 20))); break;
      }
      for (int i = 0; i < 6; ++i) s[i] = x[i];
      if (fm->cls == CRO_ALU_C_TRCP64 || fm->cls == CRO_ALU_C_TSQRT64) cro_alu_wd(s, v);
      else if (fm->cls >= CRO_ALU_C_TEXP16) s[0] = cro_alu_h_of(v);
      else s[0] = cro_alu_u((float)v);
      break;
    }
  }
}

// the eight words of a row: sources, then the expected result
static inline void cro_alu_row(uint32_t seed, int form, int row, uint32_t* words) {
  cro_alu_sources(seed, form, row, words);
  cro_alu_form(form)->ref(words, words + 6);
  if (cro_alu_form(form)->sig == CRO_ALU_SIG_V1_MBCNT)
    words[6] = cro_alu_mbcnt(words[0], words[1], words[2], (uint32_t)row);
  // words nothing compares (a transcendental's rows past its anchors) are zero
  if (row >= cro_alu_checked_rows(cro_alu_form(form)->check, form)) words[6] = words[7] = 0u;
}

// the whole table: CRO_ALU_FORM_COUNT * 64 * 8 words
static inline void cro_alu_table(uint32_t seed, uint32_t* words) {
  for (int f = 0; f < CRO_ALU_FORM_COUNT; ++f)
    for (int r = 0; r < CRO_ALU_ROWS; ++r)
      cro_alu_row(seed, f, r, words + ((size_t)f * CRO_ALU_ROWS + r) * CRO_ALU_ROW_WORDS);
}

// -- record and aggregation -------------------------------------------------------------

// One per wave and round, written by lane 0; as CroMovementRecord, the last
// word being the wave's transcendental digest.
struct CroAluRecord {
  uint32_t xcc_id;
  uint32_t hw_id;
  uint32_t fail_mask;  // bit t: check t
  uint32_t n_bad;
  uint32_t first_bad;  // cro_alu_elem of the lowest bad word; ~0 = none
  uint32_t bits_bad;
  uint32_t valid;
  union {
    uint32_t digest;
    uint32_t reserved;
  };
};

struct CroAluAgg {
  unsigned long long waves_run;
  unsigned long long waves_bad;
  unsigned long long bad[CRO_ALU_TESTS];
  int cus_seen;
  int xcds_seen;
  int simds_seen;
  int cus_bad;
  int xcd, se, sh, cu, simd;
  unsigned int fail_mask;
  unsigned int first_fail_mask;
  unsigned int n_bad;
  unsigned int first_bad;
  unsigned int bits_bad;
  long long first_bad_index;
  unsigned int digest;        // the majority digest; 0 where there is none
  unsigned int no_majority;   // 1: no digest is held by a strict majority
  unsigned long long digest_waves;  // waves that hold the majority digest
};

// The digest a strict majority of the valid records holds (Boyer-Moore, then
// a count); a record that deviates gets the transcendental bit on a private
// copy (and, where nothing else failed in it, first_bad ~0 and the xor of the
// digests as bits_bad); with no strict majority every valid record is flagged.
// Then cro_wave_summarize.
static inline void cro_alu_aggregate(const CroAluRecord* records, size_t n, CroAluAgg* out) {
  uint32_t cand = 0;
  size_t votes = 0, valid = 0, hold = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!records[i].valid) continue;
    ++valid;
    if (!votes) { cand = records[i].digest; votes = 1; }
    else if (records[i].digest == cand) ++votes;
    else --votes;
  }
  for (size_t i = 0; i < n; ++i) hold += records[i].valid && records[i].digest == cand;
  const bool majority = 2 * hold > valid;
  CroAluRecord* copy = n ? new CroAluRecord[n] : nullptr;
  for (size_t i = 0; i < n; ++i) {
    copy[i] = records[i];
    if (!copy[i].valid || (majority && copy[i].digest == cand)) continue;
    if (!copy[i].fail_mask) {
      copy[i].n_bad = 1;
      copy[i].first_bad = ~0u;
      copy[i].bits_bad = majority ? copy[i].digest ^ cand : 0u;
    }
    copy[i].fail_mask |= 1u << CRO_ALU_TRANS;
  }
  CroWaveSummary s;
  cro_wave_summarize(copy, n, &s);
  delete[] copy;
  cro_wave_common(s, out);
  for (int t = 0; t < CRO_ALU_TESTS; ++t) out->bad[t] = s.bad[t];
  out->fail_mask = s.fail_mask;
  out->digest = majority && valid ? cand : 0u;
  out->no_majority = valid && !majority;
  out->digest_waves = majority ? hold : 0;
}

// -- C ABI (libcroalu.so) ---------------------------------------------------------------

// Zero takes the library default.  The selftest_* options are for tests: they
// alter data only, in bounds.  selftest_elem is cro_alu_elem(form, word, row,
// lane); the row must be the one the lane takes in some repeat of the run.
//   mode 1  bit selftest_bit of the EXPECTED word of that element of check
//           selftest_test is flipped in every wave (with selftest_also = 1 +
//           form2 the same word, row and lane of form2, a form of another
//           check, as well); of the transcendental check only an anchor row
//   mode 2  that bit of the COMPUTED word is flipped on the waves whose CU key
//           (cro_cov_cu_key) is selftest_key; a non-anchor row of the
//           transcendental check changes those waves' digest
struct CroAluOpts {
  int grid_blocks;
  int iters;
  int max_rounds;
  unsigned int seed;
  int selftest_mode;
  int selftest_test;
  int selftest_bit;
  unsigned int selftest_elem;
  unsigned int selftest_key;
  int selftest_also;
  double min_cu_fraction;  // > 0: fewer CUs seen than this fraction is rc -39
};

struct CroAluResult {
  int ok;
  int rc;  // 0 ok, -1 HIP error or bad argument, -38 mismatch, -39 CU-coverage floor
  int cus_expected;
  int rounds;
  struct CroAluAgg agg;
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

int cro_alu_run(int device, const struct CroAluOpts* opts, struct CroAluResult* out);

// cro_alu_run, and the rounds' raw records (at most max_records), round-major.
int cro_alu_run_records(int device, const struct CroAluOpts* opts, struct CroAluResult* out,
                        struct CroAluRecord* records_out, int max_records);

// One wave of the stage's own device code for `form` on 64 caller rows: `in`
// is 64 rows of six source words (1536 bytes), `out` receives 64 rows of two
// raw result words (512 bytes).  0 ok, -10 bad argument, -1 HIP error.
int cro_alu_tile(int device, int form, const void* in, int n_in_bytes, void* out,
                 int n_out_bytes);

#ifdef __cplusplus
}
#endif
