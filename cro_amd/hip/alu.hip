// cro_amd gfx950 ALU probe stage: exact checks of the vector ALU (integer,
// bit, packed, dot, f32, f16, f64, conversions, scaled conversions, compares)
// and of the scalar ALU on every CU and SIMD, with fault location, and a
// consensus check of the transcendental unit.
//
// The shape of the formats and movement stages: one 256-thread workgroup per
// CU (a CU's whole dynamic LDS is requested for placement only), four waves,
// one per SIMD.  Each wave runs every form of croalu.h `iters` times: at
// repeat r lane l loads row (l + r) & 63 of the form's operand table (the
// scalar forms row r & 63, made uniform with v_readfirstlane_b32), runs the
// form's asm statement and compares every result word with the table by a
// plain integer compare.  Nothing is computed on the device but the
// instruction under test.  Mismatches are counted per wave and check with a
// ballot; the transcendental forms' results are also folded into a per-wave
// digest.  Each wave reads where it ran (XCC_ID, HW_ID) and lane 0 writes one
// CroAluRecord.  No workgroup waits for another.
//
// Wait states.  One instruction per statement wherever possible, so defs and
// uses are operands the compiler sees.  The statements with more than one
// (carry chains through VCC, SCC captures, the compare read back through
// v_cndmask_b32, v_cmpx with its masked move and the EXEC restore) carry
// their own s_nop; every scalar statement opens with s_nop 4 because its
// operands come from v_readfirstlane_b32.  Every statement names vcc and scc
// as clobbered; the v_cmpx one saves EXEC in a scratch SGPR pair that is its
// operand and restores it (the compiler reserves exec: it cannot be named).
// Scalar results reach the comparison and the record through a VGPR
// (v_mov_b32).  The stage holds no scalar memory write of any kind.
//
// cro_alu_tile runs one wave of the same exec_form<> on caller rows, which is
// how the tests prove every reference of croalu.h.
//
// A library of its own (libcroalu.so): host plumbing from crohost.h.

#include <hip/hip_runtime.h>
#include <cstring>
#include <utility>
#include <vector>

#include "croalu.h"
#include "crohost.h"

namespace {

constexpr int kWaves = kBlock / 64;
// ≈0.048 ms per repeat on an MI355X: 8 is the largest power of two whose
// median (0.389 ms) does not exceed the compute stage's (0.572 ms; 16 repeats
// cost 0.772 ms: profiles/alu_probe_mi355x.md)
constexpr int kDefaultIters = 8;
constexpr int kDefaultRounds = 4;
constexpr int kMaxRounds = 64;
constexpr int kMaxGrid = 1 << 16;
constexpr int kMaxIters = 1 << 12;
constexpr size_t kTableWords = (size_t)CRO_ALU_FORM_COUNT * CRO_ALU_ROWS * CRO_ALU_ROW_WORDS;

extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
typedef uint32_t u32x32 __attribute__((ext_vector_type(32)));
typedef uint32_t u32x6 __attribute__((ext_vector_type(6)));

// -- per-form constants ---------------------------------------------------------------

struct FormInfo {
  int check, sig, nres;
  bool scalar;
};

constexpr int sig_nres(int sig) {
  constexpr int nres[CRO_ALU_SIG_COUNT] = {
#define CRO_ALU_X(name, ns, nr) nr,
      CRO_ALU_SIGS(CRO_ALU_X)
#undef CRO_ALU_X
  };
  return nres[sig];
}

constexpr FormInfo kForms[CRO_ALU_FORM_COUNT] = {
#define CRO_ALU_X(check, name, mnem, tmpl, sig, cls)                      \
  {CRO_ALU_##check, CRO_ALU_SIG_##sig, sig_nres(CRO_ALU_SIG_##sig),       \
   CRO_ALU_SIG_##sig >= CRO_ALU_SIG_S1_S},
    CRO_ALU_FORMS(CRO_ALU_X)
#undef CRO_ALU_X
};

// -- the statements, one macro per signature --------------------------------------------
// s[0..5] are the row's source words, w[0..1] receive the raw result.

#define U64(lo, hi) (((uint64_t)(hi) << 32) | (uint64_t)(lo))
#define OUT64(v) w[0] = (uint32_t)(v), w[1] = (uint32_t)((v) >> 32)
#define CLOB "vcc", "scc"
#define UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#define SOPEN "s_nop 4\n\t"
#define TOV(dst, src) asm volatile("v_mov_b32 %0, %1" : "=v"(dst) : "s"(src))

#define ALU_V1_V(t) asm volatile(t : "=v"(w[0]) : "v"(s[0]) : CLOB);
#define ALU_V1_VV(t) asm volatile(t : "=v"(w[0]) : "v"(s[0]), "v"(s[1]) : CLOB);
#define ALU_V1_VVV(t) asm volatile(t : "=v"(w[0]) : "v"(s[0]), "v"(s[1]), "v"(s[2]) : CLOB);
#define ALU_V1_VVO(t) w[0] = s[2]; asm volatile(t : "+v"(w[0]) : "v"(s[0]), "v"(s[1]) : CLOB);
#define ALU_V1_VVVO(t) w[0] = s[3]; asm volatile(t : "+v"(w[0]) : "v"(s[0]), "v"(s[1]), "v"(s[2]) : CLOB);
// lo mask, hi mask, base; the second instruction reads the first's result
#define ALU_V1_MBCNT(t) asm volatile(t : "=&v"(w[0]) : "v"(s[0]), "v"(s[1]), "v"(s[2]) : CLOB);
#define ALU_V2_D(t) { uint64_t r; asm volatile(t : "=v"(r) : "v"(U64(s[0], s[1])) : CLOB); OUT64(r); }
#define ALU_V2_DD(t) { uint64_t r; asm volatile(t : "=v"(r) : "v"(U64(s[0], s[1])), "v"(U64(s[2], s[3])) : CLOB); OUT64(r); }
#define ALU_V2_DDD(t) { uint64_t r; asm volatile(t : "=v"(r) : "v"(U64(s[0], s[1])), "v"(U64(s[2], s[3])), "v"(U64(s[4], s[5])) : CLOB); OUT64(r); }
#define ALU_V2_VD(t) { uint64_t r; asm volatile(t : "=v"(r) : "v"(s[0]), "v"(U64(s[1], s[2])) : CLOB); OUT64(r); }
#define ALU_V2_DV(t) { uint64_t r; asm volatile(t : "=v"(r) : "v"(U64(s[0], s[1])), "v"(s[2]) : CLOB); OUT64(r); }
#define ALU_V2_VVD(t) { uint64_t r; asm volatile(t : "=v"(r) : "v"(s[0]), "v"(s[1]), "v"(U64(s[2], s[3])) : CLOB); OUT64(r); }
#define ALU_V2_V(t) { uint64_t r; asm volatile(t : "=v"(r) : "v"(s[0]) : CLOB); OUT64(r); }
#define ALU_V2_VV(t) { uint64_t r; asm volatile(t : "=v"(r) : "v"(s[0]), "v"(s[1]) : CLOB); OUT64(r); }
#define ALU_V1_D(t) asm volatile(t : "=v"(w[0]) : "v"(U64(s[0], s[1])) : CLOB);
#define ALU_V1_DD(t) asm volatile(t : "=v"(w[0]) : "v"(U64(s[0], s[1])), "v"(U64(s[2], s[3])) : CLOB);
#define ALU_V1_DV(t) asm volatile(t : "=v"(w[0]) : "v"(U64(s[0], s[1])), "v"(s[2]) : CLOB);
#define ALU_V2C_VVVV(t) asm volatile(t : "=&v"(w[0]), "=&v"(w[1]) : "v"(s[0]), "v"(s[1]), "v"(s[2]), "v"(s[3]) : CLOB);
// %1 holds EXEC across the masked move (exec itself cannot be named: the
// compiler reserves it; the statement leaves it as it found it)
#define ALU_V1_CMPX(t) { uint64_t keep; w[0] = s[2]; asm volatile(t : "+v"(w[0]), "=&s"(keep) : "v"(s[0]), "v"(s[1]) : CLOB); }
// plain C++ on operands the compiler cannot see through: the full IEEE
// divide (v_div_scale / v_rcp / v_div_fmas / v_div_fixup) and square root
#define ALU_X_DIV(t) { double x = __builtin_bit_cast(double, U64(s[0], s[1])), y = __builtin_bit_cast(double, U64(s[2], s[3])); \
    asm volatile("" : "+v"(x), "+v"(y)); const uint64_t r = __builtin_bit_cast(uint64_t, x / y); OUT64(r); }
#define ALU_X_SQRT(t) { double x = __builtin_bit_cast(double, U64(s[0], s[1])); asm volatile("" : "+v"(x)); \
    const uint64_t r = __builtin_bit_cast(uint64_t, __dsqrt_rn(x)); OUT64(r); }
// 32 result registers, folded (rotate-left-5 and xor, even and odd) in plain C++
#define ALU_V2_FP6(t) { u32x6 a; u32x32 r; _Pragma("unroll") for (int i = 0; i < 6; ++i) a[i] = s[i]; \
    asm volatile(t : "=&v"(r) : "v"(a) : CLOB); w[0] = w[1] = 0; \
    _Pragma("unroll") for (int i = 0; i < 32; ++i) w[i & 1] = ((w[i & 1] << 5) | (w[i & 1] >> 27)) ^ r[i]; }
#define ALU_S1_S(t) { uint32_t r; asm volatile(SOPEN t : "=s"(r) : "s"(UNI(s[0])) : CLOB); TOV(w[0], r); }
#define ALU_S1_SS(t) { uint32_t r; asm volatile(SOPEN t : "=s"(r) : "s"(UNI(s[0])), "s"(UNI(s[1])) : CLOB); TOV(w[0], r); }
#define ALU_S1_SSSS(t) { uint32_t r; asm volatile(SOPEN t : "=s"(r) : "s"(UNI(s[0])), "s"(UNI(s[1])), "s"(UNI(s[2])), "s"(UNI(s[3])) : CLOB); TOV(w[0], r); }
#define ALU_S1C_S(t) { uint32_t r, c; asm volatile(SOPEN t : "=s"(r), "=s"(c) : "s"(UNI(s[0])) : CLOB); TOV(w[0], r); TOV(w[1], c); }
#define ALU_S1C_SS(t) { uint32_t r, c; asm volatile(SOPEN t : "=s"(r), "=s"(c) : "s"(UNI(s[0])), "s"(UNI(s[1])) : CLOB); TOV(w[0], r); TOV(w[1], c); }
#define ALU_S2C_SSSS(t) { uint32_t r, c; asm volatile(SOPEN t : "=&s"(r), "=&s"(c) : "s"(UNI(s[0])), "s"(UNI(s[1])), "s"(UNI(s[2])), "s"(UNI(s[3])) : CLOB); TOV(w[0], r); TOV(w[1], c); }
#define UNI64(lo, hi) U64(UNI(lo), UNI(hi))
#define TOV64(r) { const uint32_t lo = (uint32_t)(r), hi = (uint32_t)((r) >> 32); TOV(w[0], lo); TOV(w[1], hi); }
#define ALU_S2_Q(t) { uint64_t r; asm volatile(SOPEN t : "=s"(r) : "s"(UNI64(s[0], s[1])) : CLOB); TOV64(r); }
#define ALU_S2_QQ(t) { uint64_t r; asm volatile(SOPEN t : "=s"(r) : "s"(UNI64(s[0], s[1])), "s"(UNI64(s[2], s[3])) : CLOB); TOV64(r); }
#define ALU_S2_QS(t) { uint64_t r; asm volatile(SOPEN t : "=s"(r) : "s"(UNI64(s[0], s[1])), "s"(UNI(s[2])) : CLOB); TOV64(r); }
#define ALU_S1C_Q(t) { uint32_t r, c; asm volatile(SOPEN t : "=&s"(r), "=s"(c) : "s"(UNI64(s[0], s[1])) : CLOB); TOV(w[0], r); TOV(w[1], c); }
// SCC alone: the instruction's own result goes to scratch SGPRs
#define ALU_SC_QQ(t) { uint32_t c; uint64_t r; asm volatile(SOPEN t : "=&s"(c), "=&s"(r) : "s"(UNI64(s[0], s[1])), "s"(UNI64(s[2], s[3])) : CLOB); TOV(w[0], c); }
#define ALU_SC_QS(t) { uint32_t c; uint64_t r; asm volatile(SOPEN t : "=&s"(c), "=&s"(r) : "s"(UNI64(s[0], s[1])), "s"(UNI(s[2])) : CLOB); TOV(w[0], c); }
#define ALU_SC_SSSS(t) { uint32_t c, lo, hi; asm volatile(SOPEN t : "=&s"(c), "=&s"(lo), "=&s"(hi) : "s"(UNI(s[0])), "s"(UNI(s[1])), "s"(UNI(s[2])), "s"(UNI(s[3])) : CLOB); TOV(w[0], c); }
#define ALU_S1_Q(t) { uint32_t r; asm volatile(SOPEN t : "=s"(r) : "s"(UNI64(s[0], s[1])) : CLOB); TOV(w[0], r); }

// the one place a form's instruction is executed: stage and tile call it
template <int F>
__device__ inline void exec_form(const uint32_t (&s)[6], uint32_t (&w)[2]);

#define CRO_ALU_X(check, name, mnem, tmpl, sig, cls)                                        \
  template <>                                                                               \
  __device__ inline void exec_form<CRO_ALU_FORM_##name>(const uint32_t (&s)[6],            \
                                                        uint32_t (&w)[2]) {                 \
    ALU_##sig(tmpl)                                                                         \
  }
CRO_ALU_FORMS(CRO_ALU_X)
#undef CRO_ALU_X

// calls f(std::integral_constant<int, F>) for every form
template <class Fn, int... F>
__device__ inline void each_form_impl(Fn&& f, std::integer_sequence<int, F...>) {
  (f(std::integral_constant<int, F>{}), ...);
}
template <class Fn>
__device__ inline void each_form(Fn&& f) {
  each_form_impl(f, std::make_integer_sequence<int, CRO_ALU_FORM_COUNT>{});
}

template <class Fn>
__device__ inline void each_check(Fn&& f) {
  each_form_impl(f, std::make_integer_sequence<int, CRO_ALU_TESTS>{});
}

// row `row` of form F: sources and expected words
__device__ inline void load_row(const uint4* table, int form, uint32_t row, uint32_t (&s)[6],
                                uint32_t (&want)[2]) {
  const uint4* p = table + ((size_t)form * CRO_ALU_ROWS + row) * 2;
  const uint4 lo = p[0], hi = p[1];
  s[0] = lo.x, s[1] = lo.y, s[2] = lo.z, s[3] = lo.w, s[4] = hi.x, s[5] = hi.y;
  want[0] = hi.z, want[1] = hi.w;
}

// ---------------------------------------------------------------------------
// raw tile entry: one wave, 64 caller rows, raw result words
// ---------------------------------------------------------------------------

template <int F>
__global__ __launch_bounds__(64) void tile_kernel(const uint32_t* in, uint32_t* out) {
  const uint32_t lane = threadIdx.x;  // exactly one wave of 64
  uint32_t s[6], w[2] = {0, 0};
  if constexpr (kForms[F].scalar) {
    for (uint32_t r = 0; r < 64; ++r) {  // every lane runs every row, lane r keeps row r
      uint32_t t[2] = {0, 0};
#pragma unroll
      for (int k = 0; k < 6; ++k) s[k] = in[r * 6 + k];
      exec_form<F>(s, t);
      if (lane == r) w[0] = t[0], w[1] = t[1];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = in[lane * 6 + k];
    exec_form<F>(s, w);
  }
  out[lane * 2] = w[0];
  out[lane * 2 + 1] = kForms[F].nres > 1 ? w[1] : 0u;
}

// ---------------------------------------------------------------------------
// stage kernel
// ---------------------------------------------------------------------------

struct AluParams {
  const uint4* table;    // CRO_ALU_FORM_COUNT * 64 rows of two uint4
  CroAluRecord* records;  // this round's grid_blocks * 4 records
  uint32_t iters;
  uint32_t inj_mode;
  uint32_t inj_form;   // the element of the self-test: form, word, row, lane
  uint32_t inj_form2;  // mode 1: a second form; ~0 = none
  uint32_t inj_word;
  uint32_t inj_row;
  uint32_t inj_lane;
  uint32_t inj_key;
  uint32_t inj_flip;
};

// What one wave found in one check (as the movement stage's).
struct Tally {
  uint32_t n_bad = 0;
  uint32_t first = ~0u;
  uint32_t bits = 0;

  __device__ void add(uint32_t diff, uint32_t elem) {
    bits |= diff;
    n_bad += (uint32_t)__popcll(__ballot(diff != 0));  // branch-free: one block per repeat
    first = diff && elem < first ? elem : first;
  }
  __device__ void reduce() {
    if (!n_bad) return;
    for (int off = 32; off > 0; off >>= 1) {
      bits |= __shfl_xor(bits, off, 64);
      const uint32_t other = __shfl_xor(first, off, 64);
      first = other < first ? other : first;
    }
  }
};

__device__ inline uint32_t rotl5(uint32_t v) { return (v << 5) | (v >> 27); }

__global__ __launch_bounds__(kBlock) void alu_kernel(AluParams p) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t xcc_id, hw_id;  // for the report only
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
  // the elements of the self-test; ~0 is no element
  const uint32_t inj_elem = cro_alu_elem((int)p.inj_form, (int)p.inj_word, (int)p.inj_row, (int)p.inj_lane);
  const uint32_t want_elem = p.inj_mode == 1 ? inj_elem : ~0u;
  const uint32_t want_elem2 =
      p.inj_mode == 1 && p.inj_form2 != ~0u
          ? cro_alu_elem((int)p.inj_form2, (int)p.inj_word, (int)p.inj_row, (int)p.inj_lane)
          : ~0u;
  const uint32_t got_elem =
      p.inj_mode == 2 && cro_cov_cu_key(xcc_id, hw_id) == p.inj_key ? inj_elem : ~0u;

  Tally t[CRO_ALU_TESTS];
  uint32_t digest = 0;
  uint32_t fence = 0;
  for (uint32_t it = 0; it < p.iters; ++it) {
    each_form([&](auto fc) {
      constexpr int F = decltype(fc)::value;
      constexpr FormInfo fi = kForms[F];
      const uint32_t row = fi.scalar ? (it & 63u) : ((lane + it) & 63u);
      // the loads of at most eight forms are in flight at a time: a zero
      // added to the table pointer (which so stays a global pointer) passes
      // through a statement ordered with the forms' own, or
      // the compiler hoists every form's loads and spills
      if constexpr (F % 8 == 0) asm volatile("" : "+s"(fence));
      uint32_t s[6], want[2], w[2] = {0, 0};
      load_row(p.table + fence, F, row, s, want);
      exec_form<F>(s, w);
#pragma unroll
      for (int k = 0; k < fi.nres; ++k) {
        // the self-test compares whole elements: they change with the repeat,
        // so nothing per form is kept across repeats
        const uint32_t elem = cro_alu_elem(F, k, (int)row, (int)lane);
        uint32_t got = w[k], exp = want[k];
        if (elem == want_elem || elem == want_elem2) exp ^= p.inj_flip;
        if (elem == got_elem) got ^= p.inj_flip;
        // the one result that depends on the lane: expected in plain C++
        if constexpr (fi.sig == CRO_ALU_SIG_V1_MBCNT) exp = cro_alu_mbcnt(s[0], s[1], s[2], lane);
        if constexpr (fi.check == CRO_ALU_TRANS) {
          digest = rotl5(digest) ^ got;
          if (row >= (uint32_t)cro_alu_checked_rows(fi.check, F)) exp = got;  // only the anchors are compared
        }
        t[fi.check].add(got ^ exp, elem);
      }
    });
  }
  for (int off = 32; off > 0; off >>= 1) digest = rotl5(digest) ^ __shfl_xor(digest, off, 64);

  uint32_t fail_mask = 0, n_bad = 0, first_bad = ~0u, bits_bad = 0;
  // (a fold, not a loop: t[] must stay in registers)
  each_check([&](auto kc) {
    constexpr int k = CRO_ALU_TESTS - 1 - decltype(kc)::value;
    t[k].reduce();
    if (t[k].n_bad) {  // the lowest failing check leads
      fail_mask |= 1u << k;
      n_bad = t[k].n_bad;
      first_bad = t[k].first;
      bits_bad = t[k].bits;
    }
  });
  if (lane == 0) {
    CroAluRecord rec;
    rec.xcc_id = xcc_id;
    rec.hw_id = hw_id;
    rec.fail_mask = fail_mask;
    rec.n_bad = n_bad;
    rec.first_bad = first_bad;
    rec.bits_bad = bits_bad;
    rec.valid = 1;
    rec.digest = digest;
    p.records[blockIdx.x * kWaves + wave] = rec;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// Per-device cached context: the operand table is built and uploaded when the
// seed changes, not per call; the record buffer grows on demand.
struct AluCtx : CtxBase {
  int cus = 0;
  uint32_t* d_table = nullptr;
  bool table_ready = false;
  uint32_t table_seed = 0;
  RecordBuf<CroAluRecord> records;
};
AluCtx g_actx[kMaxDevices];

int prepare(AluCtx* ctx, int device, uint32_t seed, CroAluResult* out) {
  if (!ctx->ready) {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, device));
    ctx->cus = prop.multiProcessorCount;
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(alu_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               CRO_COV_MAX_LDS_BYTES));
    // a call that failed half-way is taken up where it stopped: nothing twice
    if (!ctx->e0) CHECK(hipEventCreate(&ctx->e0));
    if (!ctx->e1) CHECK(hipEventCreate(&ctx->e1));
    if (!ctx->d_table) CHECK(hipMalloc(&ctx->d_table, kTableWords * 4));
    ctx->ready = 1;
  }
  if (!ctx->table_ready || ctx->table_seed != seed) {
    std::vector<uint32_t> table(kTableWords);
    cro_alu_table(seed, table.data());
    ctx->table_ready = false;
    CHECK(hipMemcpy(ctx->d_table, table.data(), kTableWords * 4, hipMemcpyHostToDevice));
    ctx->table_ready = true;
    ctx->table_seed = seed;
  }
  return 0;
}

// the repeat in which `lane` takes `row` of `form`
int repeat_of(int form, uint32_t row, uint32_t lane) {
  return kForms[form].scalar ? (int)row : (int)((row - lane) & 63u);
}

bool elem_ok(int form, int test, uint32_t word, uint32_t row, uint32_t lane, int iters, int mode) {
  if (form < 0 || form >= CRO_ALU_FORM_COUNT || kForms[form].check != test) return false;
  if ((int)word >= kForms[form].nres || repeat_of(form, row, lane) >= iters) return false;
  return !(mode == 1 && row >= (uint32_t)cro_alu_checked_rows(test, form));
}

int run_alu(int device, const CroAluOpts* opts, CroAluResult* out, CroAluRecord* records_out,
            int max_records) {
  CroAluOpts o;
  memset(&o, 0, sizeof(o));
  if (opts) o = *opts;
  if (o.grid_blocks < 0 || o.grid_blocks > kMaxGrid) return bad_arg(out, "grid_blocks");
  if (o.iters < 0 || o.iters > kMaxIters) return bad_arg(out, "iters");
  if (o.max_rounds < 0 || o.max_rounds > kMaxRounds) return bad_arg(out, "max_rounds");
  // as the movement stage: a floor above 1 is how the tests reach rc -39
  if (!(o.min_cu_fraction >= 0.0 && o.min_cu_fraction <= 2.0))
    return bad_arg(out, "min_cu_fraction");
  const int iters = o.iters ? o.iters : kDefaultIters;
  const int max_rounds = o.max_rounds ? o.max_rounds : kDefaultRounds;

  AluParams p;
  memset(&p, 0, sizeof(p));
  p.iters = (uint32_t)iters;
  p.inj_form2 = ~0u;
  // the self-test only ever names an element that exists
  if (o.selftest_mode < 0 || o.selftest_mode > 2) return bad_arg(out, "selftest_mode");
  if (o.selftest_mode) {
    if (o.selftest_test < 0 || o.selftest_test >= CRO_ALU_TESTS)
      return bad_arg(out, "selftest_test");
    if (o.selftest_bit < 0 || o.selftest_bit > 31) return bad_arg(out, "selftest_bit");
    const uint32_t e = o.selftest_elem;
    p.inj_mode = (uint32_t)o.selftest_mode;
    p.inj_form = e >> 13;
    p.inj_word = (e >> 12) & 1u;
    p.inj_row = (e >> 6) & 63u;
    p.inj_lane = e & 63u;
    p.inj_key = o.selftest_key;
    p.inj_flip = 1u << o.selftest_bit;
    if (!elem_ok((int)p.inj_form, o.selftest_test, p.inj_word, p.inj_row, p.inj_lane, iters,
                 o.selftest_mode))
      return bad_arg(out, "selftest_elem");
    if (o.selftest_also) {
      const int f2 = o.selftest_also - 1;
      if (o.selftest_mode != 1 || f2 < 0 || f2 >= CRO_ALU_FORM_COUNT ||
          kForms[f2].check == o.selftest_test ||
          !elem_ok(f2, kForms[f2].check, p.inj_word, p.inj_row, p.inj_lane, iters, 1))
        return bad_arg(out, "selftest_also");
      p.inj_form2 = (uint32_t)f2;
    }
  } else if (o.selftest_also) {
    return bad_arg(out, "selftest_also");
  }

  std::unique_lock<std::mutex> lock;
  AluCtx* ctx = enter_device(g_actx, device, lock, out->msg, sizeof(out->msg));
  if (ctx == nullptr) return -1;
  if (prepare(ctx, device, o.seed, out) != 0) return -1;
  const int grid = o.grid_blocks ? o.grid_blocks : ctx->cus;
  if (grid < 1) return bad_arg(out, "device reports no compute units");
  const size_t per_round = (size_t)grid * kWaves;
  CHECK(ctx->records.reserve(per_round * (size_t)max_rounds));
  out->cus_expected = ctx->cus;
  out->grid_blocks = grid;
  out->iters = iters;
  p.table = reinterpret_cast<const uint4*>(ctx->d_table);

  const auto launch = [&](CroAluRecord* d_round) {
    p.records = d_round;
    hipLaunchKernelGGL(alu_kernel, dim3(grid), dim3(kBlock), (size_t)CRO_COV_MAX_LDS_BYTES, 0, p);
  };
  if (run_rounds(*ctx, ctx->records.d, ctx->cus, per_round, max_rounds, launch,
                 cro_alu_aggregate, out, records_out, max_records) != 0)
    return -1;
  const CroAluAgg& a = out->agg;
  if (a.waves_bad) {
    snprintf(out->failed_test, sizeof(out->failed_test), "%s",
             cro_alu_test_name(a.first_fail_mask));
    const CroAluForm* fm = a.first_bad == ~0u ? nullptr : cro_alu_form((int)(a.first_bad >> 13));
    if (fm)
      snprintf(out->msg, sizeof(out->msg),
               "alu mismatch in %s at xcd=%d se=%d sh=%d cu=%d simd=%d: form %s word %u row %u "
               "lane %u, bits 0x%08x; %llu of %llu waves bad on %d CUs",
               out->failed_test, a.xcd, a.se, a.sh, a.cu, a.simd, fm->name,
               (a.first_bad >> 12) & 1u, (a.first_bad >> 6) & 63u, a.first_bad & 63u, a.bits_bad,
               a.waves_bad, a.waves_run, a.cus_bad);
    else
      snprintf(out->msg, sizeof(out->msg),
               "alu mismatch in %s at xcd=%d se=%d sh=%d cu=%d simd=%d: %s; %llu of %llu waves "
               "bad on %d CUs",
               out->failed_test, a.xcd, a.se, a.sh, a.cu, a.simd,
               a.no_majority ? "no majority digest" : "digest differs from the majority's",
               a.waves_bad, a.waves_run, a.cus_bad);
    return -38;
  }
  return coverage_floor(out, ctx->cus, o.min_cu_fraction, -39);
}

template <int F>
void launch_tile(const uint32_t* in, uint32_t* out) {
  hipLaunchKernelGGL((tile_kernel<F>), dim3(1), dim3(64), 0, 0, in, out);
}

}  // namespace

extern "C" int cro_alu_run_records(int device, const struct CroAluOpts* opts,
                                   struct CroAluResult* out, struct CroAluRecord* records_out,
                                   int max_records) {
  clear_result(out, cro_alu_aggregate);
  const double t0 = now_ms();
  out->rc = run_alu(device, opts, out, records_out, max_records);
  out->t_total_ms = now_ms() - t0;
  return out->rc;
}

extern "C" int cro_alu_run(int device, const struct CroAluOpts* opts, struct CroAluResult* out) {
  return cro_alu_run_records(device, opts, out, nullptr, 0);
}

extern "C" int cro_alu_tile(int device, int form, const void* in, int n_in_bytes, void* out,
                            int n_out_bytes) {
  constexpr int in_bytes = CRO_ALU_ROWS * 6 * 4, out_bytes = CRO_ALU_ROWS * 2 * 4;
  if (form < 0 || form >= CRO_ALU_FORM_COUNT || in == nullptr || out == nullptr) return -10;
  if (n_in_bytes != in_bytes || n_out_bytes != out_bytes) return -10;
  if (hipSetDevice(device) != hipSuccess) return -1;
  DevBuf<uint32_t> d_in, d_out;
  const auto run = [&]() -> hipError_t {
    TRY(d_in.alloc((size_t)in_bytes));
    TRY(d_out.alloc((size_t)out_bytes));
    TRY(hipMemcpy(d_in.get(), in, (size_t)in_bytes, hipMemcpyHostToDevice));
    TRY(hipMemset(d_out.get(), 0, (size_t)out_bytes));
    switch (form) {
#define CRO_ALU_X(check, name, mnem, tmpl, sig, cls) \
  case CRO_ALU_FORM_##name: launch_tile<CRO_ALU_FORM_##name>(d_in.get(), d_out.get()); break;
      CRO_ALU_FORMS(CRO_ALU_X)
#undef CRO_ALU_X
      default: return hipErrorInvalidValue;
    }
    TRY(hipGetLastError());
    return hipMemcpy(out, d_out.get(), (size_t)out_bytes, hipMemcpyDeviceToHost);
  };
  return run() == hipSuccess ? 0 : -1;
}
