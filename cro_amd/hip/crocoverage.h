// Compute-coverage probe: the per-wave record, its decode, the aggregation
// over all records of a run, and the inputs and expected tiles of the three
// matrix checks.
//
// One definition shared by the device kernel and host driver (coverage.hip),
// the native agent (agent/croagent.cpp, through croprobe.h) and a host-only
// test program, so "what the GPU compares against", "what the host reports"
// and the numpy mirrors in nodeops/probe.py cannot drift apart.  Plain C++:
// a host compiler without HIP can include it.
//
// Where a wave ran comes from two hardware registers the kernel reads with
// s_getreg_b32: XCC_ID (bits 3:0 = the XCD) and HW_ID, whose fields on this
// family are
//
//   WAVE_ID 3:0 | SIMD_ID 5:4 | PIPE_ID 7:6 | CU_ID 11:8 | SH_ID 12 | SE_ID 15:13
//
// A CU is identified by (XCD, SE, SH, CU): the "CU key" below.  The field
// positions are checked by measurement, not by trust: on a healthy MI355X
// the distinct keys must number multiProcessorCount and each key must show
// exactly the SIMD ids 0..3 (tests/test_probe_compute_gpu.py).  The location
// is used for reporting only — no result depends on where a wave ran.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define CRO_COV_HD __host__ __device__
#else
#define CRO_COV_HD
#endif

// -- tests and tile shapes ----------------------------------------------------

enum {
  CRO_COV_TEST_F32 = 0,   // v_mfma_f32_16x16x4_f32, K = 64
  CRO_COV_TEST_I8 = 1,    // v_mfma_i32_16x16x64_i8, K = 256
  CRO_COV_TEST_BF16 = 2,  // v_mfma_f32_32x32x16_bf16, K = 64
  CRO_COV_TEST_LDS = 3,   // LDS march, pattern and complement
  CRO_COV_TESTS = 4,
};

enum {
  CRO_COV_F32_K = 64,
  CRO_COV_I8_K = 256,
  CRO_COV_BF16_K = 64,
  CRO_COV_F32_ELEMS = 16 * 16,    // element index = row * 16 + col
  CRO_COV_I8_ELEMS = 16 * 16,     // element index = row * 16 + col
  CRO_COV_BF16_ELEMS = 32 * 32,   // element index = row * 32 + col
  CRO_COV_MAX_LDS_BYTES = 163840  // one CU's whole LDS
};

static inline const char* cro_cov_test_name(uint32_t fail_mask) {
  if (fail_mask & 1u) return "mfma_f32";
  if (fail_mask & 2u) return "mfma_i8";
  if (fail_mask & 4u) return "mfma_bf16";
  if (fail_mask & 8u) return "lds";
  return "";
}

// -- record ---------------------------------------------------------------------

// One per wave and round, written by lane 0.  n_bad sums over the failing
// tests; first_bad and bits_bad belong to the failing test with the lowest
// mask bit (the one cro_cov_test_name names): the element index of a matrix
// tile, or the 32-bit word offset in the workgroup's LDS.
struct CroCoverageRecord {
  uint32_t xcc_id;     // raw XCC_ID register
  uint32_t hw_id;      // raw HW_ID register
  uint32_t fail_mask;  // bit 0 f32, bit 1 i8, bit 2 bf16, bit 3 LDS
  uint32_t n_bad;      // values that differed
  uint32_t first_bad;  // lowest bad element / word offset; ~0 = none
  uint32_t bits_bad;   // OR of got ^ want over the bad values
  uint32_t valid;      // 1 once a wave wrote the record
  uint32_t reserved;
};

struct CroCoverageLoc {
  uint32_t xcd, se, sh, cu, simd, wave_slot;
};

// (XCD, SE, SH, CU) in one word: XCC_ID in bits 19:16, HW_ID bits 15:8 as is.
CRO_COV_HD static inline uint32_t cro_cov_cu_key(uint32_t xcc_id, uint32_t hw_id) {
  return ((xcc_id & 0xFu) << 16) | (hw_id & 0xFF00u);
}

static inline CroCoverageLoc cro_cov_decode(uint32_t xcc_id, uint32_t hw_id) {
  CroCoverageLoc loc;
  loc.xcd = xcc_id & 0xFu;
  loc.wave_slot = hw_id & 0xFu;
  loc.simd = (hw_id >> 4) & 0x3u;
  loc.cu = (hw_id >> 8) & 0xFu;
  loc.sh = (hw_id >> 12) & 0x1u;
  loc.se = (hw_id >> 13) & 0x7u;
  return loc;
}

static inline CroCoverageLoc cro_cov_decode_key(uint32_t key) {
  return cro_cov_decode(key >> 16, key & 0xFF00u);
}

// -- aggregation ----------------------------------------------------------------
// The per-wave stages (compute here, matrix formats in croformats.h, data
// movement in cromovement.h) write records of one layout, CroCoverageRecord's,
// and aggregate them the same way: one pass in record order into the neutral
// summary below, from which each stage fills its own Cro*Agg.

enum { CRO_COV_MAX_BAD_KEYS = 8, CRO_COV_MAX_MASK_BITS = 32 };

struct CroWaveSummary {
  unsigned long long waves_run;  // valid records
  unsigned long long waves_bad;  // records with a non-zero fail mask
  unsigned long long bad[CRO_COV_MAX_MASK_BITS];  // bad waves per fail-mask bit
  long long first_bad_index;  // index of the first bad record; -1 = none
  int cus_seen;               // distinct CU keys
  int xcds_seen;
  int simds_seen;  // distinct (CU key, SIMD) pairs
  int cus_bad;     // distinct CU keys with a bad wave
  // the first bad wave (lowest record index, i.e. lowest (round, record));
  // -1 / 0 when there is none
  int xcd, se, sh, cu, simd;
  unsigned int fail_mask;  // OR of every valid record's fail mask
  unsigned int first_fail_mask;
  unsigned int n_bad;
  unsigned int first_bad;
  unsigned int bits_bad;
  int n_bad_cu_keys;  // min(cus_bad, 8)
  unsigned int bad_cu_keys[CRO_COV_MAX_BAD_KEYS];  // in order of first appearance
};

static inline void cro_wave_summary_clear(CroWaveSummary* out) {
  memset(out, 0, sizeof(*out));
  out->first_bad_index = -1;
  out->xcd = out->se = out->sh = out->cu = out->simd = -1;
  out->first_bad = ~0u;
}

// Deterministic: one pass in record order.
template <class Record>
void cro_wave_summarize(const Record* records, size_t n, CroWaveSummary* out) {
  static_assert(sizeof(Record) == sizeof(CroCoverageRecord) &&
                    offsetof(Record, xcc_id) == offsetof(CroCoverageRecord, xcc_id) &&
                    offsetof(Record, hw_id) == offsetof(CroCoverageRecord, hw_id) &&
                    offsetof(Record, fail_mask) == offsetof(CroCoverageRecord, fail_mask) &&
                    offsetof(Record, n_bad) == offsetof(CroCoverageRecord, n_bad) &&
                    offsetof(Record, first_bad) == offsetof(CroCoverageRecord, first_bad) &&
                    offsetof(Record, bits_bad) == offsetof(CroCoverageRecord, bits_bad) &&
                    offsetof(Record, valid) == offsetof(CroCoverageRecord, valid) &&
                    offsetof(Record, reserved) == offsetof(CroCoverageRecord, reserved),
                "a per-wave stage's record has CroCoverageRecord's layout");
  // compact key: xcd(4) | se(3) | sh(1) | cu(4) = 12 bits
  static const int kKeys = 1 << 12;
  unsigned char simds[kKeys];  // bits 0..3 SIMD seen, bit 7 CU had a bad wave
  unsigned char xcds[16];
  memset(simds, 0, sizeof(simds));
  memset(xcds, 0, sizeof(xcds));
  cro_wave_summary_clear(out);
  for (size_t i = 0; i < n; ++i) {
    const Record& r = records[i];
    if (!r.valid) continue;
    ++out->waves_run;
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
    for (int t = 0; t < CRO_COV_MAX_MASK_BITS; ++t)
      if (r.fail_mask & (1u << t)) ++out->bad[t];
    if (!(simds[idx] & 0x80u)) {
      simds[idx] |= 0x80u;
      if (out->cus_bad < CRO_COV_MAX_BAD_KEYS)
        out->bad_cu_keys[out->n_bad_cu_keys++] = cro_cov_cu_key(r.xcc_id, r.hw_id);
      ++out->cus_bad;
    }
    if (out->first_bad_index < 0) {
      out->first_bad_index = (long long)i;
      out->xcd = (int)loc.xcd;
      out->se = (int)loc.se;
      out->sh = (int)loc.sh;
      out->cu = (int)loc.cu;
      out->simd = (int)loc.simd;
      out->first_fail_mask = r.fail_mask;
      out->n_bad = r.n_bad;
      out->first_bad = r.first_bad;
      out->bits_bad = r.bits_bad;
    }
  }
}

// Zeroes *out and fills what every stage's aggregate has under the same
// name; the stage adds its per-test counts and its extras.
template <class Agg>
void cro_wave_common(const CroWaveSummary& s, Agg* out) {
  memset(out, 0, sizeof(*out));
  out->waves_run = s.waves_run;
  out->waves_bad = s.waves_bad;
  out->first_bad_index = s.first_bad_index;
  out->cus_seen = s.cus_seen;
  out->xcds_seen = s.xcds_seen;
  out->simds_seen = s.simds_seen;
  out->cus_bad = s.cus_bad;
  out->xcd = s.xcd;
  out->se = s.se;
  out->sh = s.sh;
  out->cu = s.cu;
  out->simd = s.simd;
  out->first_fail_mask = s.first_fail_mask;
  out->n_bad = s.n_bad;
  out->first_bad = s.first_bad;
  out->bits_bad = s.bits_bad;
}

struct CroCoverageAgg {
  unsigned long long waves_run;  // as CroWaveSummary's
  unsigned long long waves_bad;
  unsigned long long bad_f32;  // bad waves per test, from the fail mask
  unsigned long long bad_i8;
  unsigned long long bad_bf16;
  unsigned long long bad_lds;
  long long first_bad_index;
  int cus_seen;
  int xcds_seen;
  int simds_seen;
  int cus_bad;
  int xcd, se, sh, cu, simd;
  unsigned int first_fail_mask;
  unsigned int n_bad;
  unsigned int first_bad;
  unsigned int bits_bad;
  int n_bad_cu_keys;
  unsigned int bad_cu_keys[CRO_COV_MAX_BAD_KEYS];
};

// Over no records this is the cleared aggregate.  cus_expected is carried by
// the caller's result; the aggregate itself only counts what it saw.
static inline void cro_coverage_aggregate(const CroCoverageRecord* records, size_t n,
                                          int cus_expected, CroCoverageAgg* out) {
  (void)cus_expected;
  CroWaveSummary s;
  cro_wave_summarize(records, n, &s);
  cro_wave_common(s, out);
  out->bad_f32 = s.bad[CRO_COV_TEST_F32];
  out->bad_i8 = s.bad[CRO_COV_TEST_I8];
  out->bad_bf16 = s.bad[CRO_COV_TEST_BF16];
  out->bad_lds = s.bad[CRO_COV_TEST_LDS];
  out->n_bad_cu_keys = s.n_bad_cu_keys;
  memcpy(out->bad_cu_keys, s.bad_cu_keys, sizeof(out->bad_cu_keys));
}

// -- inputs and expected tiles ----------------------------------------------------
// All three input sets come from one LCG so the numpy mirror is a few lines.
// The quick probe (probe.hip) takes its inputs and expected tile from here
// too: cro_cov_make_f32 at seed 0 and cro_cov_ref_f32.

static inline uint32_t cro_cov_lcg(uint32_t* s) {
  *s = *s * 1664525u + 1013904223u;
  return *s;
}

// A 16x64, B 64x16, row-major, values in [-0.5, 0.5)
static inline void cro_cov_make_f32(uint32_t seed, float* A, float* B) {
  uint32_t s = 0x9e3779b9u ^ seed;
  for (int i = 0; i < 16 * CRO_COV_F32_K; ++i)
    A[i] = ((float)(cro_cov_lcg(&s) >> 8) / 16777216.0f) - 0.5f;
  for (int i = 0; i < CRO_COV_F32_K * 16; ++i)
    B[i] = ((float)(cro_cov_lcg(&s) >> 8) / 16777216.0f) - 0.5f;
}

// gfx950's f32-input MFMA is bitwise a k-ordered fmaf chain, so this tile is
// compared exactly.
static inline void cro_cov_ref_f32(const float* A, const float* B, float* D) {
  for (int r = 0; r < 16; ++r)
    for (int c = 0; c < 16; ++c) {
      float acc = 0.f;
      for (int k = 0; k < CRO_COV_F32_K; ++k)
        acc = fmaf(A[r * CRO_COV_F32_K + k], B[k * 16 + c], acc);
      D[r * 16 + c] = acc;
    }
}

// A 16x256, B 256x16, row-major, the whole int8 range; both extremes are
// pinned into row 0 / column 0 so (-128)*(-128) and 127*127 are summed.
static inline void cro_cov_make_i8(uint32_t seed, int8_t* A, int8_t* B) {
  uint32_t s = 0x85ebca6bu ^ seed;
  for (int i = 0; i < 16 * CRO_COV_I8_K; ++i) A[i] = (int8_t)(uint8_t)(cro_cov_lcg(&s) >> 24);
  for (int i = 0; i < CRO_COV_I8_K * 16; ++i) B[i] = (int8_t)(uint8_t)(cro_cov_lcg(&s) >> 24);
  A[0] = -128;
  A[1] = 127;
  B[0] = -128;
  B[16] = 127;
}

// exact: |sum| <= 256 * 128 * 128 = 2^22
static inline void cro_cov_ref_i8(const int8_t* A, const int8_t* B, int32_t* D) {
  for (int r = 0; r < 16; ++r)
    for (int c = 0; c < 16; ++c) {
      int32_t acc = 0;
      for (int k = 0; k < CRO_COV_I8_K; ++k)
        acc += (int32_t)A[r * CRO_COV_I8_K + k] * (int32_t)B[k * 16 + c];
      D[r * 16 + c] = acc;
    }
}

// A 32x64, B 64x32, row-major, as bf16 bit patterns of integers in
// [-8, 8] \ {0}.  Random signs and magnitudes: neither matrix equals its
// transpose on any square block, so a swapped index shows.
static inline uint16_t cro_cov_bf16_bits(int v) {
  float f = (float)v;  // |v| <= 8: exact in bf16, the low 16 bits are zero
  uint32_t u;
  memcpy(&u, &f, sizeof(u));
  return (uint16_t)(u >> 16);
}

static inline int cro_cov_small_int(uint32_t* s) {
  const uint32_t x = cro_cov_lcg(s);
  const int mag = 1 + (int)((x >> 28) & 7u);
  return (x >> 27) & 1u ? -mag : mag;
}

static inline void cro_cov_make_bf16(uint32_t seed, int* Ai, int* Bi, uint16_t* A, uint16_t* B) {
  uint32_t s = 0xc2b2ae35u ^ seed;
  for (int i = 0; i < 32 * CRO_COV_BF16_K; ++i) {
    Ai[i] = cro_cov_small_int(&s);
    A[i] = cro_cov_bf16_bits(Ai[i]);
  }
  for (int i = 0; i < CRO_COV_BF16_K * 32; ++i) {
    Bi[i] = cro_cov_small_int(&s);
    B[i] = cro_cov_bf16_bits(Bi[i]);
  }
}

// every product and partial sum is an integer of magnitude <= 64 * 64 = 4096:
// exact in f32 in any summation order
static inline void cro_cov_ref_bf16(const int* Ai, const int* Bi, float* D) {
  for (int r = 0; r < 32; ++r)
    for (int c = 0; c < 32; ++c) {
      int acc = 0;
      for (int k = 0; k < CRO_COV_BF16_K; ++k) acc += Ai[r * CRO_COV_BF16_K + k] * Bi[k * 32 + c];
      D[r * 32 + c] = (float)acc;
    }
}
