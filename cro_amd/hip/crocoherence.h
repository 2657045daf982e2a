// Coherence probe stage: exact checks of the atomic units (L2 / memory and
// LDS) and of cross-CU, cross-XCD visibility, with fault location.
//
// Everything the host decides lives here: the contribution every lane makes
// to every tally, closed forms of a workgroup's totals, the fold of those
// totals into the XCD and device lines through the records' block -> XCD map,
// the payload hash of the visibility check, the per-wave record, the
// aggregation and the C ABI of libcrocoherence.so.  Plain C++: a host compiler
// without HIP can include it.  nodeops/coherence.py mirrors it in numpy.
//
// A launch is one epoch (1, 2, .. iters); a round is `iters` launches of the
// same grid on freshly initialised buffers.  No workgroup ever waits for
// another: every inter-workgroup dependency is resolved by the value an
// atomic returns.
//
// Checks, in fail-mask bit order (cro_coh_test_name):
//
//   0 add_u32  1 add_u64  2 add_f32  3 add_f64  4 pk_add_f16  5 pk_add_bf16
//   6 minmax   7 bitwise      tallies: non-returning agent-scope atomics on
//                             three levels of lines, compared by the host
//   8 ticket   9 cas          returning atomics, judged per wave
//   10 lds_rmw                the workgroup's LDS read-modify-write units
//   11 visibility             "whoever arrived before me is visible to me"
//
// Tally lines.  A unit is 32 64-bit words (two 128-byte lines of its own);
// words 0..17 are the slots below, 32-bit slots use the low half:
//
//   0 add_u32  1 add_u64  2 add_f32  3 add_f64  4 pk_add_f16  5 pk_add_bf16
//   6 min_u32  7 max_u32  8 min_i32  9 max_i32  10 min_f64  11 max_f64
//   12 and_u32  13 or_u32  14 xor_u32  15 and_u64  16 or_u64  17 xor_u64
//
// Units of one epoch: one per workgroup (four waves contend), 16 XCD ids x
// 16 sub-slots (the XCD the wave found itself on by XCC_ID, sub-slot
// (block >> 3) & 15) and 16 device-wide sub-slots.  The sub-slots bound what
// one slot can receive to 64 workgroups at the largest grid (1024) however
// the blocks are placed, which keeps the float tallies exact:
//
//   f32   every lane, |x| <= 511:       64 * 256 * 511 < 2^24
//   f64   every lane, |x| < 2^39:       64 * 256 * 2^39 < 2^53
//   f16   workgroup line 64 lanes <= 16 (sum <= 1024); XCD / device line one
//         lane per wave <= 8:           64 * 4 * 8 = 2048
//   bf16  workgroup line 16 lanes <= 8 (sum <= 128); XCD / device line one
//         lane per workgroup <= 4:      64 * 4 = 256
//
// All contributions are integers, so every partial sum is exact in any order.
//
// Instructions (hipcc --offload-arch=gfx950 -O3, read in the stage's assembly):
//   global_atomic_add, global_atomic_add_x2, global_atomic_add_f32,
//   global_atomic_add_f64, global_atomic_pk_add_f16, global_atomic_pk_add_bf16,
//   global_atomic_umin / umax / smin / smax, global_atomic_min_f64 / max_f64,
//   global_atomic_and / or / xor and their _x2 forms (none returning);
//   returning global_atomic_add, global_atomic_cmpswap, global_atomic_cmpswap_x2,
//   global_atomic_swap, global_atomic_or_x2; in LDS ds_add_u32, ds_add_u64,
//   ds_add_f32, ds_add_f64, ds_min_u32, ds_max_u32, ds_min_i32, ds_max_i32,
//   ds_min_f64, ds_max_f64, ds_and_b32, ds_or_b32, ds_xor_b32, ds_and_b64,
//   ds_or_b64, ds_xor_b64 and ds_cmpst_rtn_b32; no compare-and-swap loop.
//
// Not covered: LDS packed f16 / bf16 adds, system-scope and host-visible
// (fine-grained) memory, the sc1 write-through hand-off forms,
// buffer-addressed atomics, and rates.
#pragma once

#include "crocoverage.h"

enum {
  CRO_COH_ADD_U32 = 0,
  CRO_COH_ADD_U64 = 1,
  CRO_COH_ADD_F32 = 2,
  CRO_COH_ADD_F64 = 3,
  CRO_COH_PK_F16 = 4,
  CRO_COH_PK_BF16 = 5,
  CRO_COH_MINMAX = 6,
  CRO_COH_BITWISE = 7,
  CRO_COH_TICKET = 8,
  CRO_COH_CAS = 9,
  CRO_COH_LDS = 10,
  CRO_COH_VIS = 11,
  CRO_COH_TESTS = 12,
  CRO_COH_TALLIES = 8,  // checks 0..7 are tallies
};

enum {
  CRO_COH_BLOCK = 256,
  CRO_COH_MAX_GRID = 1024,
  CRO_COH_MAX_ITERS = 64,
  CRO_COH_UNIT_WORDS = 32,  // 64-bit words of a unit (256 bytes)
  CRO_COH_SLOTS = 18,       // of which are slots
  CRO_COH_XCD_IDS = 16,     // XCC_ID is a 4-bit field
  CRO_COH_SUBS = 16,        // sub-slots of the XCD and device levels
  CRO_COH_GROUP = 64,       // workgroups per arrival word
  CRO_COH_PAYLOAD = 64,     // dwords a workgroup publishes (256 bytes)
  CRO_COH_CAS_STRIDE = 32,  // dwords between two lanes' private lines (128 bytes)
  CRO_COH_LEVEL_WG = 0,
  CRO_COH_LEVEL_XCD = 1,
  CRO_COH_LEVEL_DEV = 2,
};

static const char* const kCroCohTestNames[CRO_COH_TESTS] = {
    "add_u32", "add_u64", "add_f32", "add_f64", "pk_add_f16", "pk_add_bf16",
    "minmax",  "bitwise", "ticket",  "cas",     "lds_rmw",    "visibility"};

static inline const char* cro_coh_test_name(uint32_t fail_mask) {
  for (int t = 0; t < CRO_COH_TESTS; ++t)
    if (fail_mask & (1u << t)) return kCroCohTestNames[t];
  return "";
}

// the check a slot of a unit belongs to
CRO_COV_HD static inline int cro_coh_slot_test(int slot) {
  return slot < 6 ? slot : slot < 12 ? CRO_COH_MINMAX : CRO_COH_BITWISE;
}

static inline int cro_coh_units(int grid) {
  return grid + CRO_COH_XCD_IDS * CRO_COH_SUBS + CRO_COH_SUBS;
}
CRO_COV_HD static inline uint32_t cro_coh_sub(uint32_t block) { return (block >> 3) & 15u; }
CRO_COV_HD static inline uint32_t cro_coh_xcd_unit(uint32_t grid, uint32_t xcc_id, uint32_t block) {
  return grid + (xcc_id & 15u) * CRO_COH_SUBS + cro_coh_sub(block);
}
CRO_COV_HD static inline uint32_t cro_coh_dev_unit(uint32_t grid, uint32_t block) {
  return grid + CRO_COH_XCD_IDS * CRO_COH_SUBS + cro_coh_sub(block);
}
// level of a unit index, and what it names: the block, the XCD or the sub-slot
static inline int cro_coh_unit_level(int grid, int unit, int* name) {
  if (unit < grid) {
    *name = unit;
    return CRO_COH_LEVEL_WG;
  }
  if (unit < grid + CRO_COH_XCD_IDS * CRO_COH_SUBS) {
    *name = (unit - grid) / CRO_COH_SUBS;
    return CRO_COH_LEVEL_XCD;
  }
  *name = unit - grid - CRO_COH_XCD_IDS * CRO_COH_SUBS;
  return CRO_COH_LEVEL_DEV;
}

// -- what a lane contributes -------------------------------------------------------
// g = block * 256 + tid is the lane's global id; salt = cro_coh_salt(seed, epoch).

CRO_COV_HD static inline uint32_t cro_coh_lcg(uint32_t s) { return s * 1664525u + 1013904223u; }

CRO_COV_HD static inline uint32_t cro_coh_salt(uint32_t seed, uint32_t epoch) {
  return cro_coh_lcg(cro_coh_lcg(seed ^ (epoch * 0x9e3779b9u)));
}

CRO_COV_HD static inline uint32_t cro_coh_v_u32(uint32_t g, uint32_t salt) {
  return g * 2654435761u + (salt | 1u);
}
// above 2^32, so the carry between the halves is exercised
CRO_COV_HD static inline uint64_t cro_coh_v_u64(uint32_t g) {
  return (uint64_t)(g + 1u) * 0x39E3779B1ull;
}
CRO_COV_HD static inline int cro_coh_v_f32(uint32_t block, uint32_t tid) {
  const int k = 1 + (int)tid + (int)(block & 255u);
  return (tid & 3u) == 3u ? -k : k;
}
CRO_COV_HD static inline int64_t cro_coh_v_f64(uint32_t g) {
  const int64_t k = (int64_t)(g + 1u) * 2097143;
  return (g & 3u) == 3u ? -k : k;
}
// packed adds: kind 0 f16, 1 bf16; wide 0 the workgroup line, 1 the XCD and
// device lines.  One lane in P takes part with lo = 1 + q % M, hi = M + 1 - lo
// (M even: the halves always differ), q = g / P.
CRO_COV_HD static inline void cro_coh_pk_rule(int kind, int wide, uint32_t* P, uint32_t* M) {
  if (kind == 0) {
    *P = wide ? 64u : 4u;
    *M = wide ? 8u : 16u;
  } else {
    *P = wide ? 256u : 16u;
    *M = wide ? 4u : 8u;
  }
}
CRO_COV_HD static inline bool cro_coh_pk(int kind, int wide, uint32_t block, uint32_t tid,
                                         uint32_t* lo, uint32_t* hi) {
  uint32_t P, M;
  cro_coh_pk_rule(kind, wide, &P, &M);
  if (tid % P != block % P) return false;
  const uint32_t q = (block * 256u + tid) / P;
  *lo = 1u + q % M;
  *hi = M + 1u - *lo;
  return true;
}
// the lane of a workgroup that takes part in both packed adds at both widths
// (self-test mode 2 drops its adds)
CRO_COV_HD static inline uint32_t cro_coh_drop_tid(int test, uint32_t block) {
  return test == CRO_COH_PK_F16 ? block % 64u : test == CRO_COH_PK_BF16 ? block % 256u : 0u;
}
// odd lanes have the top bit set: signed and unsigned order differ
CRO_COV_HD static inline uint32_t cro_coh_v_mm32(uint32_t g) {
  return ((g & 1u) << 31) | (g * 8u + 5u);
}
CRO_COV_HD static inline int64_t cro_coh_v_mmf64(uint32_t g) {
  const int64_t k = (int64_t)(g + 1u) * 2097143;
  return (g & 1u) ? -k : k;
}
CRO_COV_HD static inline uint32_t cro_coh_mask_and(uint32_t block, uint32_t salt) {
  return ((block + 1u) * 0x9E3779B1u) ^ salt;
}
CRO_COV_HD static inline uint32_t cro_coh_mask_or(uint32_t block, uint32_t salt) {
  return ((block + 1u) * 0x85EBCA6Bu) ^ salt;
}
CRO_COV_HD static inline uint32_t cro_coh_rotl13(uint32_t x) { return (x << 13) | (x >> 19); }
CRO_COV_HD static inline uint32_t cro_coh_v_and32(uint32_t block, uint32_t tid, uint32_t salt) {
  return ~(cro_coh_mask_and(block, salt) & (1u << (tid & 31u)));
}
CRO_COV_HD static inline uint32_t cro_coh_v_or32(uint32_t block, uint32_t tid, uint32_t salt) {
  return cro_coh_mask_or(block, salt) & (1u << (tid & 31u));
}
CRO_COV_HD static inline uint32_t cro_coh_v_xor32(uint32_t g) { return cro_coh_rotl13(g + 1u); }
CRO_COV_HD static inline uint64_t cro_coh_v_and64(uint32_t block, uint32_t tid, uint32_t salt) {
  return ~((uint64_t)(cro_coh_mask_and(block, salt) & (1u << (tid & 31u))) << 20);
}
CRO_COV_HD static inline uint64_t cro_coh_v_or64(uint32_t block, uint32_t tid, uint32_t salt) {
  return (uint64_t)(cro_coh_mask_or(block, salt) & (1u << (tid & 31u))) << 24;
}
CRO_COV_HD static inline uint64_t cro_coh_v_xor64(uint32_t g) {
  return ((uint64_t)(g + 1u) << 32) | (uint32_t)~(g + 1u);
}

// compare-and-swap lines: what lane g's words hold after epoch e (0 before the first)
CRO_COV_HD static inline uint32_t cro_coh_cas32(uint32_t epoch, uint32_t g) {
  return epoch ? (g + 1u) * 0x9E3779B1u + epoch * 0x7F4A7C15u : 0u;
}
CRO_COV_HD static inline uint64_t cro_coh_cas64(uint32_t epoch, uint32_t g) {
  return epoch ? (uint64_t)(g + 1u) * 0x9E3779B97F4A7C15ull + (uint64_t)epoch * 0xD1B54A32D192ED03ull
               : 0ull;
}
CRO_COV_HD static inline uint32_t cro_coh_xchg32(uint32_t epoch, uint32_t g) {
  return epoch ? cro_coh_cas32(epoch, g) ^ 0xA5A5A5A5u : 0u;
}

// visibility payload: dword idx of producer block in epoch e (0: what the host writes)
CRO_COV_HD static inline uint32_t cro_coh_payload(uint32_t seed, uint32_t epoch, uint32_t block,
                                                  uint32_t idx) {
  uint32_t s = cro_coh_salt(seed, epoch) ^ ((block * CRO_COH_PAYLOAD + idx) * 0x9e3779b9u);
  s = cro_coh_lcg(s);
  return cro_coh_lcg(s);
}

// -- a workgroup's totals -----------------------------------------------------------

// logical values of the 18 slots (float slots as the integers they hold)
struct CroCohTotals {
  uint32_t add32;
  uint64_t add64;
  int64_t f32, f64;
  int32_t f16_lo, f16_hi, bf16_lo, bf16_hi;
  uint32_t min_u, max_u;
  int32_t min_i, max_i;
  int64_t min_f, max_f;
  uint32_t and32, or32, xor32;
  uint64_t and64, or64, xor64;
};

static const int64_t kCroCohF64Far = (int64_t)1 << 60;  // beyond every f64 min / max operand

static inline void cro_coh_totals_init(CroCohTotals* t) {
  memset(t, 0, sizeof(*t));
  t->min_u = 0xFFFFFFFFu;
  t->max_u = 0u;
  t->min_i = 0x7FFFFFFF;
  t->max_i = (int32_t)0x80000000u;
  t->min_f = kCroCohF64Far;
  t->max_f = -kCroCohF64Far;
  t->and32 = 0xFFFFFFFFu;
  t->and64 = ~0ull;
}

// one lane's contributions folded in, exactly what the kernel's lane does;
// skip_test >= 0 leaves that check's operations out (self-test mode 2)
static inline void cro_coh_totals_lane(CroCohTotals* t, uint32_t block, uint32_t tid, uint32_t salt,
                                       int wide, int skip_test) {
  const uint32_t g = block * 256u + tid;
  uint32_t lo, hi;
  if (skip_test != CRO_COH_ADD_U32) t->add32 += cro_coh_v_u32(g, salt);
  if (skip_test != CRO_COH_ADD_U64) t->add64 += cro_coh_v_u64(g);
  if (skip_test != CRO_COH_ADD_F32) t->f32 += cro_coh_v_f32(block, tid);
  if (skip_test != CRO_COH_ADD_F64) t->f64 += cro_coh_v_f64(g);
  if (skip_test != CRO_COH_PK_F16 && cro_coh_pk(0, wide, block, tid, &lo, &hi)) {
    t->f16_lo += (int32_t)lo;
    t->f16_hi += (int32_t)hi;
  }
  if (skip_test != CRO_COH_PK_BF16 && cro_coh_pk(1, wide, block, tid, &lo, &hi)) {
    t->bf16_lo += (int32_t)lo;
    t->bf16_hi += (int32_t)hi;
  }
  if (skip_test != CRO_COH_MINMAX) {
    const uint32_t w = cro_coh_v_mm32(g);
    const int64_t x = cro_coh_v_mmf64(g);
    if (w < t->min_u) t->min_u = w;
    if (w > t->max_u) t->max_u = w;
    if ((int32_t)w < t->min_i) t->min_i = (int32_t)w;
    if ((int32_t)w > t->max_i) t->max_i = (int32_t)w;
    if (x < t->min_f) t->min_f = x;
    if (x > t->max_f) t->max_f = x;
  }
  if (skip_test != CRO_COH_BITWISE) {
    t->and32 &= cro_coh_v_and32(block, tid, salt);
    t->or32 |= cro_coh_v_or32(block, tid, salt);
    t->xor32 ^= cro_coh_v_xor32(g);
    t->and64 &= cro_coh_v_and64(block, tid, salt);
    t->or64 |= cro_coh_v_or64(block, tid, salt);
    t->xor64 ^= cro_coh_v_xor64(g);
  }
}

// brute force: every lane of the block in turn
static inline void cro_coh_block_totals_brute(uint32_t block, uint32_t salt, int wide,
                                              CroCohTotals* t) {
  cro_coh_totals_init(t);
  for (uint32_t tid = 0; tid < 256u; ++tid) cro_coh_totals_lane(t, block, tid, salt, wide, -1);
}

// xor of 0 .. n
static inline uint32_t cro_coh_xor_upto(uint32_t n) {
  switch (n & 3u) {
    case 0: return n;
    case 1: return 1u;
    case 2: return n + 1u;
    default: return 0u;
  }
}

// sum over j < n of 1 + (q0 + j) % M
static inline uint32_t cro_coh_cycle_sum(uint32_t q0, uint32_t n, uint32_t M) {
  const uint32_t full = n / M, rest = n % M;
  uint32_t sum = full * (M * (M + 1u) / 2u);
  for (uint32_t j = 0; j < rest; ++j) sum += 1u + (q0 + j) % M;
  return sum;
}

// closed forms of the same totals
static inline void cro_coh_block_totals(uint32_t block, uint32_t salt, int wide, CroCohTotals* t) {
  const uint32_t base = block * 256u;
  const int64_t K = 2097143;
  t->add32 = 2654435761u * (256u * base + 32640u) + 256u * (salt | 1u);
  t->add64 = 0x39E3779B1ull * (256ull * base + 32896ull);
  t->f32 = 16256 + 128 * (int64_t)(block & 255u);
  t->f64 = K * (128 * (int64_t)base + 16256);
  for (int kind = 0; kind < 2; ++kind) {
    uint32_t P, M;
    cro_coh_pk_rule(kind, wide, &P, &M);
    const uint32_t n = 256u / P;
    const int32_t lo = (int32_t)cro_coh_cycle_sum(n * block, n, M);
    const int32_t hi = (int32_t)(n * (M + 1u)) - lo;
    if (kind == 0) {
      t->f16_lo = lo;
      t->f16_hi = hi;
    } else {
      t->bf16_lo = lo;
      t->bf16_hi = hi;
    }
  }
  t->min_u = base * 8u + 5u;
  t->max_u = 0x80000000u | ((base + 255u) * 8u + 5u);
  t->min_i = (int32_t)(0x80000000u | ((base + 1u) * 8u + 5u));
  t->max_i = (int32_t)((base + 254u) * 8u + 5u);
  t->min_f = -(int64_t)(base + 256u) * K;
  t->max_f = (int64_t)(base + 255u) * K;
  const uint32_t xr = cro_coh_xor_upto(base + 256u) ^ cro_coh_xor_upto(base);
  t->and32 = ~cro_coh_mask_and(block, salt);
  t->or32 = cro_coh_mask_or(block, salt);
  t->xor32 = cro_coh_rotl13(xr);
  t->and64 = ~((uint64_t)cro_coh_mask_and(block, salt) << 20);
  t->or64 = (uint64_t)cro_coh_mask_or(block, salt) << 24;
  t->xor64 = ((uint64_t)xr << 32) | xr;  // an even count: the complements cancel
}

// a workgroup's totals folded into a line shared with others
static inline void cro_coh_totals_fold(CroCohTotals* acc, const CroCohTotals* b) {
  acc->add32 += b->add32;
  acc->add64 += b->add64;
  acc->f32 += b->f32;
  acc->f64 += b->f64;
  acc->f16_lo += b->f16_lo;
  acc->f16_hi += b->f16_hi;
  acc->bf16_lo += b->bf16_lo;
  acc->bf16_hi += b->bf16_hi;
  if (b->min_u < acc->min_u) acc->min_u = b->min_u;
  if (b->max_u > acc->max_u) acc->max_u = b->max_u;
  if (b->min_i < acc->min_i) acc->min_i = b->min_i;
  if (b->max_i > acc->max_i) acc->max_i = b->max_i;
  if (b->min_f < acc->min_f) acc->min_f = b->min_f;
  if (b->max_f > acc->max_f) acc->max_f = b->max_f;
  acc->and32 &= b->and32;
  acc->or32 |= b->or32;
  acc->xor32 ^= b->xor32;
  acc->and64 &= b->and64;
  acc->or64 |= b->or64;
  acc->xor64 ^= b->xor64;
}

// f16 bits of an integer 0..2048
static inline uint32_t cro_coh_f16_bits(int32_t v) {
  if (v <= 0) return 0u;
  int e = 0;
  while ((v >> (e + 1)) != 0) ++e;
  const uint32_t frac = e <= 10 ? ((uint32_t)v << (10 - e)) : ((uint32_t)v >> (e - 10));
  return ((uint32_t)(e + 15) << 10) | (frac & 0x3FFu);
}
static inline uint32_t cro_coh_f32_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof(u));
  return u;
}
static inline uint64_t cro_coh_f64_bits(double d) {
  uint64_t u;
  memcpy(&u, &d, sizeof(u));
  return u;
}

// the 32 words of a unit that holds these totals (bit patterns; unused words zero)
static inline void cro_coh_encode(const CroCohTotals* t, uint64_t* w) {
  memset(w, 0, CRO_COH_UNIT_WORDS * sizeof(uint64_t));
  w[0] = t->add32;
  w[1] = t->add64;
  w[2] = cro_coh_f32_bits((float)t->f32);
  w[3] = cro_coh_f64_bits((double)t->f64);
  w[4] = cro_coh_f16_bits(t->f16_lo) | (cro_coh_f16_bits(t->f16_hi) << 16);
  w[5] = (cro_coh_f32_bits((float)t->bf16_lo) >> 16) |
         (cro_coh_f32_bits((float)t->bf16_hi) & 0xFFFF0000u);
  w[6] = t->min_u;
  w[7] = t->max_u;
  w[8] = (uint32_t)t->min_i;
  w[9] = (uint32_t)t->max_i;
  w[10] = cro_coh_f64_bits((double)t->min_f);
  w[11] = cro_coh_f64_bits((double)t->max_f);
  w[12] = t->and32;
  w[13] = t->or32;
  w[14] = t->xor32;
  w[15] = t->and64;
  w[16] = t->or64;
  w[17] = t->xor64;
}

// What every unit holds before a launch (units * 32 words).
static inline void cro_coh_initial_units(int grid, uint64_t* units) {
  CroCohTotals t;
  cro_coh_totals_init(&t);
  const int n = cro_coh_units(grid);
  for (int u = 0; u < n; ++u) cro_coh_encode(&t, units + (size_t)u * CRO_COH_UNIT_WORDS);
}

// What every unit must hold after the launch of `epoch`: closed forms per
// workgroup, folded into the XCD and device lines through xcc_of_block (the
// raw XCC_ID of each block's records).
static inline void cro_coh_expected_units(int grid, uint32_t seed, uint32_t epoch,
                                          const uint32_t* xcc_of_block, uint64_t* units) {
  const uint32_t salt = cro_coh_salt(seed, epoch);
  const int n_shared = CRO_COH_XCD_IDS * CRO_COH_SUBS + CRO_COH_SUBS;
  CroCohTotals shared[CRO_COH_XCD_IDS * CRO_COH_SUBS + CRO_COH_SUBS];
  for (int u = 0; u < n_shared; ++u) cro_coh_totals_init(&shared[u]);
  for (int b = 0; b < grid; ++b) {
    CroCohTotals own, wide;
    cro_coh_block_totals((uint32_t)b, salt, 0, &own);
    cro_coh_block_totals((uint32_t)b, salt, 1, &wide);
    cro_coh_encode(&own, units + (size_t)b * CRO_COH_UNIT_WORDS);
    cro_coh_totals_fold(&shared[cro_coh_xcd_unit(0, xcc_of_block[b], (uint32_t)b)], &wide);
    cro_coh_totals_fold(&shared[cro_coh_dev_unit(0, (uint32_t)b)], &wide);
  }
  for (int u = 0; u < n_shared; ++u)
    cro_coh_encode(&shared[u], units + (size_t)(grid + u) * CRO_COH_UNIT_WORDS);
}

// -- record -------------------------------------------------------------------------

// One per wave and launch, written by lane 0.  fail_mask holds the checks a
// wave judges itself (ticket, cas, lds_rmw, visibility); n_bad, first_bad and
// bits_bad belong to the lowest of them that failed: ticket the lane that drew
// a ticket beyond the grid, cas sub-check * 64 + lane (sub-checks: 0 hit32,
// 1 miss32, 2 hit64, 3 miss64, 4 exchange), lds_rmw the word of the LDS unit
// (32 + tid for the compare-and-swap words), visibility producer block * 64 +
// dword.  The vis_* fields are the visibility check's own.
struct CroCoherenceRecord {
  uint32_t xcc_id;
  uint32_t hw_id;
  uint32_t fail_mask;
  uint32_t n_bad;
  uint32_t first_bad;
  uint32_t bits_bad;
  uint32_t valid;
  uint32_t block;
  uint32_t vis_pairs;        // producers this wave checked
  uint32_t vis_bad;          // dwords that differed
  uint32_t vis_stale;        // of which equalled the previous epoch's value
  uint32_t vis_first_block;  // first bad producer block; ~0 = none
  uint32_t vis_first_dword;
  uint32_t vis_bits;  // OR of got ^ want over the bad dwords
  uint32_t preread;   // xor of what the pre-read consumed (keeps the loads alive)
  uint32_t epoch;
};

struct CroCoherenceAgg {
  unsigned long long waves_run;
  unsigned long long waves_bad;
  unsigned long long bad[CRO_COH_TESTS];  // per check: bad slots (tallies, ticket) or bad waves
  unsigned long long pairs_checked;       // visibility: sum of vis_pairs
  unsigned long long pairs_expected;      // sum over epochs and groups of n(n-1)/2
  unsigned long long vis_bad;
  unsigned long long vis_stale;
  unsigned long long tally_got;  // the first bad tally slot
  unsigned long long tally_want;
  long long first_bad_index;  // index of the first bad record; -1 = none
  int cus_seen;
  int xcds_seen;
  int simds_seen;
  int cus_bad;
  // the first failure's place; -1 where it does not apply
  int xcd, se, sh, cu, simd;
  unsigned int fail_mask;  // every check that failed
  unsigned int first_fail_mask;
  unsigned int n_bad;
  unsigned int first_bad;
  unsigned int bits_bad;
  int tally_level;  // 0 workgroup, 1 XCD, 2 device line; -1 = none
  int tally_slot;   // the unit's slot word 0..17
  int tally_unit;   // what the line names: block, XCD or device sub-slot
  int tally_epoch;
  int bad_block;  // the workgroup a failure names (tally workgroup line, ticket owner,
                  // visibility producer, else the failing wave's own); -1 = none
  // the first bad ticket slot: how often it was marked and the lane that drew it
  int ticket_slot;
  int ticket_epoch;
  unsigned int ticket_seen;
  unsigned int ticket_owner;
  unsigned int reserved;
};

static inline void cro_coherence_agg_clear(CroCoherenceAgg* out) {
  memset(out, 0, sizeof(*out));
  out->first_bad_index = -1;
  out->xcd = out->se = out->sh = out->cu = out->simd = -1;
  out->first_bad = ~0u;
  out->tally_level = out->tally_slot = out->tally_unit = out->tally_epoch = -1;
  out->bad_block = -1;
  out->ticket_slot = out->ticket_epoch = -1;
}

static inline void cro_coh_agg_place(CroCoherenceAgg* out, const CroCoherenceRecord* r,
                                     bool with_simd) {
  const CroCoverageLoc loc = cro_cov_decode(r->xcc_id, r->hw_id);
  out->xcd = (int)loc.xcd;
  out->se = (int)loc.se;
  out->sh = (int)loc.sh;
  out->cu = (int)loc.cu;
  out->simd = with_simd ? (int)loc.simd : -1;
}

// The records of `launches` launches of `grid` workgroups, launch-major
// (launch, block, wave).  Deterministic: one pass in record order.  Counts
// coverage, the per-wave checks and the visibility pairs; the pair count of
// every launch and 64-block group must be exactly n(n-1)/2.
static inline void cro_coherence_aggregate(const CroCoherenceRecord* records, int grid,
                                           int launches, CroCoherenceAgg* out) {
  static const int kKeys = 1 << 12;
  unsigned char simds[kKeys];
  unsigned char xcds[16];
  memset(simds, 0, sizeof(simds));
  memset(xcds, 0, sizeof(xcds));
  cro_coherence_agg_clear(out);
  const size_t per_launch = (size_t)grid * 4;
  for (int l = 0; l < launches; ++l) {
    for (int g0 = 0; g0 < grid; g0 += CRO_COH_GROUP) {
      const int n = grid - g0 < CRO_COH_GROUP ? grid - g0 : CRO_COH_GROUP;
      unsigned long long pairs = 0, want = (unsigned long long)n * (n - 1) / 2;
      bool complete = true;
      for (int b = g0; b < g0 + n; ++b)
        for (int w = 0; w < 4; ++w) {
          const size_t i = (size_t)l * per_launch + (size_t)b * 4 + w;
          const CroCoherenceRecord& r = records[i];
          if (!r.valid) {
            complete = false;
            continue;
          }
          ++out->waves_run;
          pairs += r.vis_pairs;
          out->vis_bad += r.vis_bad;
          out->vis_stale += r.vis_stale;
          const CroCoverageLoc loc = cro_cov_decode(r.xcc_id, r.hw_id);
          const unsigned idx = (loc.xcd << 8) | ((r.hw_id >> 8) & 0xFFu);
          if ((simds[idx] & 0x0Fu) == 0) ++out->cus_seen;
          if (!(simds[idx] & (1u << loc.simd))) ++out->simds_seen;
          simds[idx] |= (unsigned char)(1u << loc.simd);
          if (!xcds[loc.xcd]) ++out->xcds_seen;
          xcds[loc.xcd] = 1;
          if (!r.fail_mask) continue;
          ++out->waves_bad;
          out->fail_mask |= r.fail_mask;
          for (int t = CRO_COH_TICKET; t < CRO_COH_TESTS; ++t)
            if (r.fail_mask & (1u << t)) ++out->bad[t];
          if (!(simds[idx] & 0x80u)) {
            simds[idx] |= 0x80u;
            ++out->cus_bad;
          }
          if (out->first_bad_index < 0) {
            out->first_bad_index = (long long)i;
            cro_coh_agg_place(out, &r, true);
            out->first_fail_mask = r.fail_mask;
            out->n_bad = r.n_bad;
            out->first_bad = r.first_bad;
            out->bits_bad = r.bits_bad;
            // a visibility failure names the producer, any other the wave's own workgroup
            out->bad_block = cro_coh_test_name(r.fail_mask) == kCroCohTestNames[CRO_COH_VIS]
                                 ? (int)r.vis_first_block
                                 : (int)r.block;
          }
        }
      out->pairs_checked += pairs;
      out->pairs_expected += want;
      // a wrong pair count is a wrong value returned by the arrival fetch_or
      if (complete && pairs != want) {
        out->fail_mask |= 1u << CRO_COH_VIS;
        ++out->bad[CRO_COH_VIS];
      }
    }
  }
}

// Tally lines of one launch against the expected ones (units * 32 words each).
// Counts the bad slots per check into out->bad and keeps the first as the
// aggregate's tally_* fields (lowest epoch, then unit, then slot).  xcc and
// hw ids of each block's first record name the place of a workgroup line.
static inline int cro_coh_check_tallies(const uint64_t* got, const uint64_t* want, int grid,
                                        int epoch, const CroCoherenceRecord* launch_records,
                                        CroCoherenceAgg* out) {
  int n_bad = 0;
  const int units = cro_coh_units(grid);
  for (int u = 0; u < units; ++u)
    for (int s = 0; s < CRO_COH_SLOTS; ++s) {
      const uint64_t a = got[(size_t)u * CRO_COH_UNIT_WORDS + s];
      const uint64_t b = want[(size_t)u * CRO_COH_UNIT_WORDS + s];
      if (a == b) continue;
      const int test = cro_coh_slot_test(s);
      ++n_bad;
      ++out->bad[test];
      out->fail_mask |= 1u << test;
      if (out->tally_level >= 0) continue;
      int name = -1;
      out->tally_level = cro_coh_unit_level(grid, u, &name);
      out->tally_unit = name;
      out->tally_slot = s;
      out->tally_epoch = epoch;
      out->tally_got = a;
      out->tally_want = b;
      if (out->tally_level == CRO_COH_LEVEL_WG) {
        out->bad_block = name;
        if (launch_records[(size_t)name * 4].valid)
          cro_coh_agg_place(out, &launch_records[(size_t)name * 4], false);
      } else if (out->tally_level == CRO_COH_LEVEL_XCD) {
        out->xcd = name;
      }
    }
  return n_bad;
}

// The ticket marks of one launch: every seen word must be exactly `want_of_0`
// for slot 0 (1 but for self-test mode 1) and 1 elsewhere.  A duplicate or a
// hole counts into bad[ticket]; the first is kept with who claimed the slot.
static inline int cro_coh_check_tickets(const uint32_t* seen, const uint32_t* owner, int grid,
                                        int epoch, uint32_t want_of_0,
                                        const CroCoherenceRecord* launch_records,
                                        CroCoherenceAgg* out) {
  int n_bad = 0;
  const uint32_t n = (uint32_t)grid * 256u;
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t want = t == 0 ? want_of_0 : 1u;
    if (seen[t] == want) continue;
    ++n_bad;
    ++out->bad[CRO_COH_TICKET];
    out->fail_mask |= 1u << CRO_COH_TICKET;
    if (out->ticket_slot >= 0) continue;
    out->ticket_slot = (int)t;
    out->ticket_epoch = epoch;
    out->ticket_seen = seen[t];
    out->ticket_owner = owner[t];
    if (owner[t] < n && out->tally_level < 0) {
      out->bad_block = (int)(owner[t] >> 8);
      const CroCoherenceRecord* r = &launch_records[(size_t)(owner[t] >> 6)];
      if (r->valid) cro_coh_agg_place(out, r, true);
    }
  }
  return n_bad;
}

// The arrival words of one launch: the word of a group of n blocks must have
// exactly its n low bits set.
static inline int cro_coh_check_words(const uint64_t* words, int grid, CroCoherenceAgg* out) {
  int n_bad = 0;
  for (int g0 = 0; g0 < grid; g0 += CRO_COH_GROUP) {
    const int n = grid - g0 < CRO_COH_GROUP ? grid - g0 : CRO_COH_GROUP;
    const uint64_t want = n == 64 ? ~0ull : ((1ull << n) - 1ull);
    if (words[g0 / CRO_COH_GROUP] == want) continue;
    ++n_bad;
    ++out->bad[CRO_COH_VIS];
    out->fail_mask |= 1u << CRO_COH_VIS;
  }
  return n_bad;
}

// What the host's own comparisons found (tallies, ticket marks, arrival
// words; accumulated in an aggregate of its own) joins what the records say.
// The lowest failing check leads: where the host found it, its place is the
// host's.
static inline void cro_coh_agg_merge(CroCoherenceAgg* out, const CroCoherenceAgg* host) {
  for (int t = 0; t < CRO_COH_TESTS; ++t) out->bad[t] += host->bad[t];
  const unsigned int wave_mask = out->fail_mask;
  out->fail_mask |= host->fail_mask;
  out->tally_got = host->tally_got;
  out->tally_want = host->tally_want;
  out->tally_level = host->tally_level;
  out->tally_slot = host->tally_slot;
  out->tally_unit = host->tally_unit;
  out->tally_epoch = host->tally_epoch;
  out->ticket_slot = host->ticket_slot;
  out->ticket_epoch = host->ticket_epoch;
  out->ticket_seen = host->ticket_seen;
  out->ticket_owner = host->ticket_owner;
  const unsigned int host_low = host->fail_mask & (0u - host->fail_mask);
  const unsigned int wave_low = wave_mask & (0u - wave_mask);
  const unsigned int placed = (1u << CRO_COH_TALLIES) - 1u + (1u << CRO_COH_TICKET);
  if ((host_low & placed) && (!wave_low || host_low < wave_low)) {
    out->first_bad_index = -1;
    out->first_fail_mask = 0;
    out->xcd = host->xcd;
    out->se = host->se;
    out->sh = host->sh;
    out->cu = host->cu;
    out->simd = host->simd;
    out->bad_block = host->bad_block;
  }
}

// -- C ABI (libcrocoherence.so) -----------------------------------------------------

// Zero takes the library default.  The selftest_* options are for tests:
// wrong data, in bounds.
//   mode 1  the host flips bit selftest_bit (0..31) of the EXPECTED value of
//           check selftest_test: the stage must fail with that name
//   mode 2  the workgroup whose CU key (cro_cov_cu_key) is selftest_key
//           misbehaves in check selftest_test: a tally: one lane drops its
//           operations; visibility: bit selftest_bit of payload dword 5 is
//           flipped; lds_rmw: a bit of an LDS total is flipped; ticket: one
//           ticket is left unmarked; cas: one returned value is corrupted
//   mode 3  consumers skip the acquire fence of the visibility check (a
//           measurement: reads are then fresh or stale)
struct CroCoherenceOpts {
  int grid_blocks;  // workgroups, at most 1024; default one per CU
  int iters;        // launches (epochs) per round, at most 64
  int max_rounds;   // bounded relaunch while a CU is unseen
  unsigned int seed;
  int selftest_mode;
  int selftest_test;
  int selftest_bit;
  unsigned int selftest_key;
  double min_cu_fraction;  // > 0: fewer CUs seen than this fraction is rc -35
};

struct CroCoherenceResult {
  int ok;
  int rc;  // 0 ok, -1 HIP error or bad argument, -34 mismatch, -35 CU-coverage floor
  int cus_expected;
  int rounds;
  struct CroCoherenceAgg agg;
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

int cro_coherence_run(int device, const struct CroCoherenceOpts* opts,
                      struct CroCoherenceResult* out);

// cro_coherence_run, and of the LAST round: the raw records (at most
// max_records, launch-major) and, where units_out is not null, the tally
// units as downloaded (at most max_unit_words 64-bit words, launch-major,
// cro_coh_units(grid) * 32 words per launch).
int cro_coherence_run_records(int device, const struct CroCoherenceOpts* opts,
                              struct CroCoherenceResult* out,
                              struct CroCoherenceRecord* records_out, int max_records,
                              unsigned long long* units_out, long long max_unit_words);

#ifdef __cplusplus
}
#endif
