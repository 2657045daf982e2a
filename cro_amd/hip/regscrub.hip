// cro_amd gfx950 register scrub stage: clear and verify the vector register
// file of every SIMD of every CU before a device is drained (croregscrub.h
// says what that covers and what it does not).
//
// One kernel, 256-thread workgroups.  The kernel allocates all 512 vector
// registers per lane (its march names v255 and a255, so next_free_vgpr is 512
// and accum_offset 256); at that size one wave owns a SIMD's whole file, so a
// workgroup's four waves sit on the four SIMDs of one CU and no second
// workgroup fits beside it.  No LDS request is needed for placement.
//
// Each wave, in ONE asm statement (between two statements the compiler may use
// a clobbered register) and in uniform control flow with EXEC all ones (the
// block size guarantees full waves), on v<first>..v255 and a0..a255:
//
//   census — compare every register as found with the fill word and count the
//            lanes that differ, before the block writes any of them;
//   fill   — write the fill word to every register;
//   verify — read every register back, count the lanes that differ, keep the
//            lowest word index and the OR of got ^ fill.
//
// The text for each register comes from one list of register names
// (CRO_REG_VGPRS / CRO_REG_AGPRS) through the preprocessor.  Counts and the
// first index are kept in SGPRs (popcount and find-first of the compare mask);
// only the OR of the differing bits is per lane, and it is reduced with
// shuffles after the block.  Nothing is reduced through LDS, the block holds
// vector and scalar ALU instructions only, and every store to memory is plain
// C++ on the wave's record.  Only counts, offsets and bit masks leave the
// device.
//
// Wait states (the assembler pads nothing inside an asm statement): a v_cmp's
// VCC is read by scalar instructions only, after an s_nop 4, the longest wait
// the ISA lists for a VALU-written SGPR; VCC written by s_cselect_b64 is read
// by v_cndmask_b32 after an s_nop 0; all fills come before all verifies, so a
// v_accvgpr_write and the v_accvgpr_read of the same register are hundreds of
// instructions apart.
//
// The registers below the first covered one are the kernel's own (thread id,
// record address, the block's operands).  A last asm statement overwrites them
// with the fill word after the record is written; that is not verified.
//
// A library of its own, libcroregscrub.so (cro_amd/hip/build.py:
// build_reg_scrub); host plumbing shared with the other stages in crohost.h.

#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>

#include "crohost.h"
#include "croregscrub.h"

namespace {

constexpr int kDefaultRounds = 4;  // the bounds of the LDS stage
constexpr int kMaxRounds = 64;
constexpr int kMaxGrid = 1 << 14;
constexpr int kWaves = CRO_REG_SCRUB_WAVES;
static_assert(kBlock == 64 * kWaves, "four full waves per workgroup");

// ---------------------------------------------------------------------------
// the register lists
// ---------------------------------------------------------------------------

#define CRO_D10(F, p) \
  F(p##0) F(p##1) F(p##2) F(p##3) F(p##4) F(p##5) F(p##6) F(p##7) F(p##8) F(p##9)
#define CRO_D100(F, p)                                                              \
  CRO_D10(F, p##0) CRO_D10(F, p##1) CRO_D10(F, p##2) CRO_D10(F, p##3) CRO_D10(F, p##4) \
  CRO_D10(F, p##5) CRO_D10(F, p##6) CRO_D10(F, p##7) CRO_D10(F, p##8) CRO_D10(F, p##9)
// 20 .. 255
#define CRO_REG_20_255(F)                                                            \
  CRO_D10(F, 2) CRO_D10(F, 3) CRO_D10(F, 4) CRO_D10(F, 5) CRO_D10(F, 6) CRO_D10(F, 7) \
  CRO_D10(F, 8) CRO_D10(F, 9) CRO_D100(F, 1) CRO_D10(F, 20) CRO_D10(F, 21)           \
  CRO_D10(F, 22) CRO_D10(F, 23) CRO_D10(F, 24) F(250) F(251) F(252) F(253) F(254) F(255)

// the covered VGPRs, from CRO_REG_SCRUB_FIRST_VGPR up, and all AGPRs
#define CRO_REG_VGPRS(F) F(16) F(17) F(18) F(19) CRO_REG_20_255(F)
#define CRO_REG_AGPRS(F) \
  F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) CRO_D10(F, 1) CRO_REG_20_255(F)
// the kernel's own VGPRs, below the first covered one
#define CRO_REG_LOW_VGPRS(F) \
  F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14) F(15)
static_assert(CRO_REG_SCRUB_FIRST_VGPR == 16, "CRO_REG_VGPRS starts at the first covered VGPR");

// reg_slot as assembler expressions: VGPR n is slot n - 16, AGPR n slot 240 + n
#define CRO_VSLOT(n) "(" #n "-16)"
#define CRO_ASLOT(n) "(" #n "+240)"

// -- per-register text ----------------------------------------------------------
// Operands: see the statement in the kernel.

// vcc = the lanes of this register that the self-test addresses
#define CRO_SELECT(slot)                         \
  "s_cmp_eq_u32 %[slot], " slot "\n\t"           \
  "s_cselect_b64 vcc, %[mask], 0\n\t"            \
  "s_nop 0\n\t"
// plant: the body word (in vt2: VCC is the one scalar a VALU instruction may
// read here), the pattern (in vp) in the addressed lanes
#define CRO_PLANT_V(n) \
  CRO_SELECT(CRO_VSLOT(n)) "v_cndmask_b32 v" #n ", %[vt2], %[vp], vcc\n\t"
#define CRO_PLANT_A(n)                                                      \
  CRO_SELECT(CRO_ASLOT(n)) "v_cndmask_b32 %[vt], %[vt2], %[vp], vcc\n\t"   \
                           "v_accvgpr_write_b32 a" #n ", %[vt]\n\t"
// count the lanes of `src` that differ from the fill word into `cnt`, and keep
// the lowest slot * 64 + lane in `first`
#define CRO_TALLY(src, slot, cnt, first)            \
  "v_cmp_ne_u32 vcc, %[fill], " src "\n\t"          \
  "s_nop 4\n\t"                                     \
  "s_bcnt1_i32_b64 %[t], vcc\n\t"                   \
  "s_add_u32 " cnt ", " cnt ", %[t]\n\t"            \
  "s_ff1_i32_b64 %[t], vcc\n\t"                     \
  "s_add_u32 %[t], %[t], " slot "*64\n\t"           \
  "s_cmp_lg_u64 vcc, 0\n\t"                         \
  "s_cselect_b32 %[t], %[t], -1\n\t"                \
  "s_min_u32 " first ", " first ", %[t]\n\t"
#define CRO_CENSUS_V(n) CRO_TALLY("v" #n, CRO_VSLOT(n), "%[cn]", "%[cf]")
#define CRO_CENSUS_A(n) \
  "v_accvgpr_read_b32 %[vt], a" #n "\n\t" CRO_TALLY("%[vt]", CRO_ASLOT(n), "%[cn]", "%[cf]")
#define CRO_FILL_V(n) "v_mov_b32 v" #n ", %[fill]\n\t"
#define CRO_FILL_A(n) "v_accvgpr_write_b32 a" #n ", %[vp]\n\t"  // vp holds the fill word
// flip: xor the flip word into the addressed lanes
#define CRO_FLIP_V(n)                                  \
  CRO_SELECT(CRO_VSLOT(n))                             \
  "v_xor_b32 %[vt], %[vp], v" #n "\n\t"                \
  "v_cndmask_b32 v" #n ", v" #n ", %[vt], vcc\n\t"
#define CRO_FLIP_A(n)                                  \
  CRO_SELECT(CRO_ASLOT(n))                             \
  "v_accvgpr_read_b32 %[vt], a" #n "\n\t"              \
  "v_xor_b32 %[vt2], %[vp], %[vt]\n\t"                 \
  "v_cndmask_b32 %[vt], %[vt], %[vt2], vcc\n\t"        \
  "v_accvgpr_write_b32 a" #n ", %[vt]\n\t"
#define CRO_VERIFY_V(n)                                     \
  CRO_TALLY("v" #n, CRO_VSLOT(n), "%[vn]", "%[vf]")         \
  "v_xor_b32 %[vt], %[fill], v" #n "\n\t"                   \
  "v_or_b32 %[bits], %[bits], %[vt]\n\t"
#define CRO_VERIFY_A(n)                                     \
  "v_accvgpr_read_b32 %[vt], a" #n "\n\t"                   \
  CRO_TALLY("%[vt]", CRO_ASLOT(n), "%[vn]", "%[vf]")        \
  "v_xor_b32 %[vt], %[fill], %[vt]\n\t"                     \
  "v_or_b32 %[bits], %[bits], %[vt]\n\t"
#define CRO_CLOBBER_V(n) , "v" #n
#define CRO_CLOBBER_A(n) , "a" #n
#define CRO_LOW_FILL(n) "v_mov_b32 v" #n ", %[fill]\n\t"

// ---------------------------------------------------------------------------
// kernel
// ---------------------------------------------------------------------------

struct RegParams {
  CroRegScrubRecord* records;  // this dispatch's 4 * grid records
  uint32_t fill_word;
  uint32_t census_only;
  uint32_t mode;  // self-test, see croregscrub.h
  uint32_t pattern;
  uint32_t st_wave;
  uint32_t st_word;
  uint32_t st_flip;  // 1 << selftest_bit
};

__global__ __launch_bounds__(kBlock) void reg_scrub_kernel(RegParams p) {
  const uint32_t lane = threadIdx.x & 63;
  // wave-uniform, and provably so: the block's scalar operands
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t xcc_id, hw_id;  // for the report only
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
  CroRegScrubRecord* rec = p.records + (size_t)blockIdx.x * kWaves + wave;

  // The block's scalar inputs, each through readfirstlane: an "s" operand must
  // be provably wave-uniform, or the compiler hands the block a VGPR.
  const auto uni = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); };
  const uint32_t fill = uni(p.fill_word);
  // the self-test's one word: its slot in this wave, or none
  const bool addressed = (p.mode == 2 || p.mode == 4) && wave == p.st_wave;
  const uint32_t slot = uni(addressed ? p.st_word >> 6 : ~0u);
  const uint32_t st_lane = uni(p.st_word & 63u);
  const uint32_t plant = uni(p.mode >= 1 && p.mode <= 3 ? 1u : 0u);
  const uint32_t body = uni(p.mode == 2 ? p.fill_word : p.pattern);
  const uint32_t pattern = uni(p.pattern);
  const uint32_t flip = uni(p.st_flip);
  const uint32_t do_fill = uni(p.mode != 3 ? 1u : 0u);
  const uint32_t do_flip = uni(p.mode == 4 ? 1u : 0u);
  const uint32_t census_only = uni(p.census_only);

  unsigned long long mask;      // scalar: the addressed lane's bit
  uint32_t cn, cf, vn, vf, t;   // scalar: census and verify count and first, scratch
  uint32_t bits, vt, vt2, vp;   // vector: OR of got ^ fill per lane, scratch
  // clang-format off
  asm volatile(
      "s_mov_b32 %[cn], 0\n\t"
      "s_mov_b32 %[cf], -1\n\t"
      "s_mov_b32 %[vn], 0\n\t"
      "s_mov_b32 %[vf], -1\n\t"
      "v_mov_b32 %[bits], 0\n\t"
      "s_lshl_b64 %[mask], 1, %[stlane]\n\t"
      // self-test plant
      "s_cmp_eq_u32 %[plant], 0\n\t"
      "s_cbranch_scc1 .Lcro_reg_census_%=\n\t"
      "v_mov_b32 %[vp], %[pat]\n\t"
      "v_mov_b32 %[vt2], %[body]\n\t"
      CRO_REG_VGPRS(CRO_PLANT_V)
      CRO_REG_AGPRS(CRO_PLANT_A)
      ".Lcro_reg_census_%=:\n\t"
      CRO_REG_VGPRS(CRO_CENSUS_V)
      CRO_REG_AGPRS(CRO_CENSUS_A)
      "s_cmp_lg_u32 %[conly], 0\n\t"
      "s_cbranch_scc1 .Lcro_reg_end_%=\n\t"
      "s_cmp_eq_u32 %[dofill], 0\n\t"
      "s_cbranch_scc1 .Lcro_reg_flip_%=\n\t"
      "v_mov_b32 %[vp], %[fill]\n\t"
      CRO_REG_VGPRS(CRO_FILL_V)
      CRO_REG_AGPRS(CRO_FILL_A)
      ".Lcro_reg_flip_%=:\n\t"
      // self-test flip
      "s_cmp_eq_u32 %[doflip], 0\n\t"
      "s_cbranch_scc1 .Lcro_reg_verify_%=\n\t"
      "v_mov_b32 %[vp], %[flip]\n\t"
      CRO_REG_VGPRS(CRO_FLIP_V)
      CRO_REG_AGPRS(CRO_FLIP_A)
      ".Lcro_reg_verify_%=:\n\t"
      CRO_REG_VGPRS(CRO_VERIFY_V)
      CRO_REG_AGPRS(CRO_VERIFY_A)
      ".Lcro_reg_end_%=:\n\t"
      : [cn] "=&s"(cn), [cf] "=&s"(cf), [vn] "=&s"(vn), [vf] "=&s"(vf), [t] "=&s"(t),
        [mask] "=&s"(mask),
        [bits] "=&v"(bits), [vt] "=&v"(vt), [vt2] "=&v"(vt2), [vp] "=&v"(vp)
      : [fill] "s"(fill), [body] "s"(body), [pat] "s"(pattern), [slot] "s"(slot),
        [stlane] "s"(st_lane), [flip] "s"(flip), [plant] "s"(plant), [dofill] "s"(do_fill),
        [doflip] "s"(do_flip), [conly] "s"(census_only)
      : "vcc", "scc" CRO_REG_VGPRS(CRO_CLOBBER_V) CRO_REG_AGPRS(CRO_CLOBBER_A));
  // clang-format on
  (void)t;
  (void)mask;
  (void)vt;
  (void)vt2;
  (void)vp;

  for (int off = 32; off > 0; off >>= 1) bits |= __shfl_xor(bits, off, 64);
  if (lane == 0) {
    rec->xcc_id = xcc_id;
    rec->hw_id = hw_id;
    rec->dirty_lanes = cn;
    rec->first_dirty = cf;
    rec->n_bad = vn;
    rec->first_bad = vf;
    rec->bits_bad = bits;
    rec->valid = 1;
  }

  // the kernel's own registers: overwritten, not verified
  // clang-format off
  asm volatile(CRO_REG_LOW_VGPRS(CRO_LOW_FILL)
               :
               : [fill] "s"(fill)
               : "memory", "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10",
                 "v11", "v12", "v13", "v14", "v15");
  // clang-format on
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// Per-device cached context (CtxBase, crohost.h): the events and the record
// buffer, which grows on demand.
struct RegCtx : CtxBase {
  int cus = 0;
  CroRegScrubRecord* d_records = nullptr;
  size_t records_cap = 0;
};
RegCtx g_rctx[kMaxDevices];

int run_reg_scrub(int device, const CroRegScrubOpts* opts, CroRegScrubResult* out,
                  CroRegScrubRecord* records_out, int max_records) {
  CroRegScrubOpts o;
  memset(&o, 0, sizeof(o));
  if (opts) o = *opts;
  out->first_vgpr = CRO_REG_SCRUB_FIRST_VGPR;
  out->regs_per_lane = CRO_REG_SCRUB_REGS_PER_LANE;
  if (o.grid < 0 || o.grid > kMaxGrid) return bad_arg(out, "grid");
  if (o.max_rounds < 0 || o.max_rounds > kMaxRounds) return bad_arg(out, "max_rounds");
  if (!(o.min_simd_fraction >= 0.0 && o.min_simd_fraction <= 1.0))  // refuses a NaN too
    return bad_arg(out, "min_simd_fraction");
  const int max_rounds = o.max_rounds ? o.max_rounds : kDefaultRounds;
  if (o.selftest_mode < 0 || o.selftest_mode > 4) return bad_arg(out, "selftest_mode");
  if (o.selftest_mode) {
    if (o.selftest_pattern == o.fill_word)
      return bad_arg(out, "selftest_pattern equals fill_word");
    if (o.selftest_wave < 0 || o.selftest_wave >= kWaves) return bad_arg(out, "selftest_wave");
    if (o.selftest_bit < 0 || o.selftest_bit > 31) return bad_arg(out, "selftest_bit");
    if (o.selftest_word >= (unsigned)CRO_REG_SCRUB_WAVE_WORDS)
      return bad_arg(out, "selftest_word");
  }

  std::unique_lock<std::mutex> lock;
  RegCtx* ctx = enter_device(g_rctx, device, lock, out->msg, sizeof(out->msg));
  if (ctx == nullptr) return -1;
  if (!ctx->ready) {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, device));
    ctx->cus = prop.multiProcessorCount;
    CHECK(hipEventCreate(&ctx->e0));
    CHECK(hipEventCreate(&ctx->e1));
    ctx->ready = 1;
  }
  const int grid = o.grid ? o.grid : ctx->cus;
  if (grid < 1) return bad_arg(out, "device reports no compute units");
  const int simds = kWaves * ctx->cus;
  // the rounds' records, then the recheck's; four per workgroup
  const size_t per_dispatch = (size_t)grid * kWaves;
  const size_t n_rounds_max = per_dispatch * (size_t)max_rounds;
  const size_t n_max = n_rounds_max + per_dispatch;
  if (ctx->records_cap < n_max) {
    if (ctx->d_records) (void)hipFree(ctx->d_records);
    ctx->d_records = nullptr;
    ctx->records_cap = 0;
    CHECK(hipMalloc(&ctx->d_records, n_max * sizeof(CroRegScrubRecord)));
    ctx->records_cap = n_max;
  }
  out->simds_expected = simds;
  out->grid = grid;

  const CroRegScrubRecord clean = CRO_REG_SCRUB_CLEAN_RECORD;
  std::vector<CroRegScrubRecord> records(n_max, clean);
  CHECK(hipMemcpy(ctx->d_records, records.data(), n_max * sizeof(clean), hipMemcpyHostToDevice));

  RegParams p;
  p.fill_word = o.fill_word;
  p.census_only = 0;
  p.mode = (uint32_t)o.selftest_mode;
  p.pattern = o.selftest_pattern;
  p.st_wave = (uint32_t)o.selftest_wave;
  p.st_word = o.selftest_word;
  p.st_flip = 1u << (o.selftest_bit & 31);
  // one dispatch into the records from `first`, event-timed and copied back
  const auto dispatch = [&](size_t first) -> hipError_t {
    p.records = ctx->d_records + first;
    float ms = 0.f;
    TRY(timed_ms(*ctx, &ms, [&] {
      hipLaunchKernelGGL(reg_scrub_kernel, dim3(grid), dim3(kBlock), 0, 0, p);
    }));
    out->gpu_ms += ms;
    return hipMemcpy(records.data() + first, p.records, per_dispatch * sizeof(clean),
                     hipMemcpyDeviceToHost);
  };

  CroRegScrubAgg agg;
  int rounds = 0;
  do {
    CHECK(dispatch((size_t)rounds * per_dispatch));
    ++rounds;
    cro_reg_scrub_aggregate(records.data(), (size_t)rounds * per_dispatch, &agg);
  } while (agg.simds_seen < simds && rounds < max_rounds);
  const size_t n = (size_t)rounds * per_dispatch;
  if (records_out && max_records > 0) {
    const size_t m = n < (size_t)max_records ? n : (size_t)max_records;
    memcpy(records_out, records.data(), m * sizeof(clean));
  }
  out->rounds = rounds;
  out->simds_seen = agg.simds_seen;
  out->cus_seen = agg.cus_seen;
  out->xcds_seen = agg.xcds_seen;
  out->waves = agg.waves;
  out->bytes_scrubbed = o.selftest_mode == 3
                            ? 0ull
                            : agg.waves * (unsigned long long)CRO_REG_SCRUB_REGS_PER_LANE * 256ull;
  out->dirty_words_before = agg.dirty_words;
  out->dirty_waves = agg.dirty_waves;
  out->first_dirty_word = agg.first_dirty_word;
  out->n_bad = agg.n_bad;
  out->bad_waves = (int)agg.bad_waves;
  out->first_bad_word = agg.first_bad_word;
  out->bits_bad = agg.bits_bad;
  out->xcd = agg.xcd;
  out->se = agg.se;
  out->sh = agg.sh;
  out->cu = agg.cu;
  out->simd = agg.simd;
  out->wave = agg.wave;
  if (agg.waves != n) {
    // a wave that never wrote its record: the launch did not run to the end
    snprintf(out->msg, sizeof(out->msg), "%llu of %zu waves reported", agg.waves, n);
    return -1;
  }

  // -- recheck: what a later dispatch, and so the next tenant, would find -------
  if (!o.skip_recheck) {
    p.census_only = 1;
    p.mode = 0;
    CHECK(dispatch(n_rounds_max));
    CroRegScrubAgg re;
    cro_reg_scrub_aggregate(records.data() + n_rounds_max, per_dispatch, &re);
    if (re.waves != per_dispatch) {
      snprintf(out->msg, sizeof(out->msg), "%llu of %zu recheck waves reported", re.waves,
               per_dispatch);
      return -1;
    }
    out->recheck_dirty_words = re.dirty_words;
    if (re.dirty_words && !agg.n_bad) {
      // nothing was bad in the rounds: the first dirty recheck wave leads
      for (size_t i = n_rounds_max; i < n_max; ++i) {
        const CroRegScrubRecord& r = records[i];
        if (!r.dirty_lanes) continue;
        const CroCoverageLoc loc = cro_cov_decode(r.xcc_id, r.hw_id);
        out->xcd = (int)loc.xcd;
        out->se = (int)loc.se;
        out->sh = (int)loc.sh;
        out->cu = (int)loc.cu;
        out->simd = (int)loc.simd;
        out->wave = (int)((i - n_rounds_max) % kWaves);
        out->first_bad_word = r.first_dirty;
        break;
      }
    }
  }

  // -- gates -------------------------------------------------------------------
  if (out->n_bad || out->recheck_dirty_words) {
    snprintf(out->msg, sizeof(out->msg),
             "register residue at xcd=%d se=%d sh=%d cu=%d simd=%d: first_bad_word %u, bits "
             "0x%08x; %llu bad words in %d waves, %llu dirty at the recheck",
             out->xcd, out->se, out->sh, out->cu, out->simd, out->first_bad_word, out->bits_bad,
             out->n_bad, out->bad_waves, out->recheck_dirty_words);
    return -44;
  }
  if (o.min_simd_fraction > 0.0 &&
      (double)out->simds_seen < o.min_simd_fraction * (double)simds) {
    snprintf(out->msg, sizeof(out->msg),
             "register scrub reached %d of %d SIMDs after %d rounds, below the floor %.3f",
             out->simds_seen, simds, rounds, o.min_simd_fraction);
    return -45;
  }
  out->ok = 1;
  snprintf(out->msg, sizeof(out->msg), "ok");
  return 0;
}

}  // namespace

extern "C" int cro_reg_scrub_run_records(int device, const struct CroRegScrubOpts* opts,
                                         struct CroRegScrubResult* out,
                                         struct CroRegScrubRecord* records_out,
                                         int max_records) {
  memset(out, 0, sizeof(*out));
  out->first_dirty_word = out->first_bad_word = ~0u;
  out->xcd = out->se = out->sh = out->cu = out->simd = out->wave = -1;
  const double t0 = now_ms();
  out->rc = run_reg_scrub(device, opts, out, records_out, max_records);
  out->t_total_ms = now_ms() - t0;
  return out->rc;
}

extern "C" int cro_reg_scrub_run(int device, const struct CroRegScrubOpts* opts,
                                 struct CroRegScrubResult* out) {
  return cro_reg_scrub_run_records(device, opts, out, nullptr, 0);
}
