// cro_amd gfx950 coherence probe stage: exact checks of the atomic units in L2
// / memory and in every CU's LDS, and of cross-CU and cross-XCD visibility
// through the agent-scope release and acquire, with fault location.
//
// Shape of the compute and formats stages: one 256-thread workgroup per CU (a
// CU's whole dynamic LDS is requested for placement, a small part is used),
// four waves, one per SIMD, each wave reads where it ran (XCC_ID, HW_ID) and
// lane 0 writes one CroCoherenceRecord per launch.  One launch is one epoch;
// the host launches the same grid `iters` times on per-epoch buffers, compares
// every tally line with the closed forms of crocoherence.h and launches again,
// a bounded number of times, while some CU is still unseen.
//
// No workgroup ever waits for another: there is no spin, no poll, no
// co-residency assumption and no retry loop.  Every inter-workgroup
// dependency is the value an atomic returns (the ticket, the arrival
// fetch_or), so a launch always runs to its end.
//
// Every pointer a contended atomic goes through gets an offset of zero from a
// vector register the compiler cannot see into first: the wave-level
// combining of atomics with a uniform address would otherwise fold 64 lanes'
// operations into one, and it is the lanes' own operations that are under
// test.
//
// A library of its own (libcrocoherence.so): host plumbing from crohost.h.

#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>

#include "crocoherence.h"
#include "crohost.h"

namespace {

constexpr int kWaves = kBlock / 64;
// ≈1.1 ms per epoch on an MI355X (the operations on one shared line are
// served one after another): already one epoch costs more than the
// compute-coverage stage's default of 0.57 ms, so no power of two fits under
// it and the default is the smallest there is
// (profiles/coherence_probe_mi355x.md)
constexpr int kDefaultIters = 1;
constexpr int kDefaultRounds = 4;
constexpr int kMaxRounds = 64;

#define RLX __ATOMIC_RELAXED
#define AGENT __HIP_MEMORY_SCOPE_AGENT
#define WGRP __HIP_MEMORY_SCOPE_WORKGROUP

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

struct CohParams {
  uint64_t* units;             // this epoch's tally units
  uint32_t* ticket;            // this epoch's ticket counter, a line of its own
  uint32_t* seen;              // this epoch's marks, grid * 256
  uint32_t* owner;             // and who drew each ticket
  uint32_t* cas;               // grid * 256 lines of 32 dwords, kept across epochs
  uint32_t* payload;           // grid * 64 dwords, kept across epochs
  uint64_t* words;             // this epoch's arrival words
  const uint64_t* expect_wg;   // this epoch's expected workgroup units (the LDS check's)
  const uint64_t* init_unit;   // a unit before any operation
  CroCoherenceRecord* records;  // this epoch's grid * 4 records
  uint32_t grid, epoch, seed, salt;
  uint32_t inj_mode, inj_test, inj_key, inj_flip;
};

// hides a pointer's uniformity from the compiler (see the head of the file):
// an offset of zero in a vector register it cannot see into; the address
// space stays known, so global and LDS operations keep their own instructions
template <class T>
__device__ inline T* per_lane(T* p) {
  uint32_t zero = 0;
  asm volatile("" : "+v"(zero));
  return p + zero;
}

// the 18 slots of one unit, by non-returning agent-scope atomics; `skip` is
// the check whose operations this lane leaves out (-1: none)
__device__ inline void tally_global(uint64_t* unit, int wide, uint32_t block, uint32_t tid,
                                    uint32_t salt, int skip) {
  uint64_t* U = per_lane(unit);
  const uint32_t g = block * 256u + tid;
  if (skip != CRO_COH_ADD_U32)
    (void)__hip_atomic_fetch_add((uint32_t*)(U + 0), cro_coh_v_u32(g, salt), RLX, AGENT);
  if (skip != CRO_COH_ADD_U64)
    (void)__hip_atomic_fetch_add(U + 1, cro_coh_v_u64(g), RLX, AGENT);
  if (skip != CRO_COH_ADD_F32)
    (void)__hip_atomic_fetch_add((float*)(U + 2), (float)cro_coh_v_f32(block, tid), RLX, AGENT);
  if (skip != CRO_COH_ADD_F64)
    (void)__hip_atomic_fetch_add((double*)(U + 3), (double)cro_coh_v_f64(g), RLX, AGENT);
  uint32_t lo, hi;
  if (skip != CRO_COH_PK_F16 && cro_coh_pk(0, wide, block, tid, &lo, &hi)) {
    const f16x2 v = {(_Float16)(float)lo, (_Float16)(float)hi};
    (void)__builtin_amdgcn_global_atomic_fadd_v2f16(
        (__attribute__((address_space(1))) f16x2*)(U + 4), v);
  }
  if (skip != CRO_COH_PK_BF16 && cro_coh_pk(1, wide, block, tid, &lo, &hi)) {
    const bf16x2 v = {(__bf16)(float)lo, (__bf16)(float)hi};
    (void)__builtin_amdgcn_global_atomic_fadd_v2bf16(
        (__attribute__((address_space(1))) bf16x2*)(U + 5), v);
  }
  if (skip != CRO_COH_MINMAX) {
    const uint32_t w = cro_coh_v_mm32(g);
    const double x = (double)cro_coh_v_mmf64(g);
    (void)__hip_atomic_fetch_min((uint32_t*)(U + 6), w, RLX, AGENT);
    (void)__hip_atomic_fetch_max((uint32_t*)(U + 7), w, RLX, AGENT);
    (void)__hip_atomic_fetch_min((int32_t*)(U + 8), (int32_t)w, RLX, AGENT);
    (void)__hip_atomic_fetch_max((int32_t*)(U + 9), (int32_t)w, RLX, AGENT);
    (void)__hip_atomic_fetch_min((double*)(U + 10), x, RLX, AGENT);
    (void)__hip_atomic_fetch_max((double*)(U + 11), x, RLX, AGENT);
  }
  if (skip != CRO_COH_BITWISE) {
    (void)__hip_atomic_fetch_and((uint32_t*)(U + 12), cro_coh_v_and32(block, tid, salt), RLX, AGENT);
    (void)__hip_atomic_fetch_or((uint32_t*)(U + 13), cro_coh_v_or32(block, tid, salt), RLX, AGENT);
    (void)__hip_atomic_fetch_xor((uint32_t*)(U + 14), cro_coh_v_xor32(g), RLX, AGENT);
    (void)__hip_atomic_fetch_and(U + 15, cro_coh_v_and64(block, tid, salt), RLX, AGENT);
    (void)__hip_atomic_fetch_or(U + 16, cro_coh_v_or64(block, tid, salt), RLX, AGENT);
    (void)__hip_atomic_fetch_xor(U + 17, cro_coh_v_xor64(g), RLX, AGENT);
  }
}

// the same operations, without the packed adds, on a unit in LDS at workgroup scope
__device__ inline void tally_lds(uint64_t* unit, uint32_t block, uint32_t tid, uint32_t salt) {
  uint64_t* U = per_lane(unit);
  const uint32_t g = block * 256u + tid;
  (void)__hip_atomic_fetch_add((uint32_t*)(U + 0), cro_coh_v_u32(g, salt), RLX, WGRP);
  (void)__hip_atomic_fetch_add(U + 1, cro_coh_v_u64(g), RLX, WGRP);
  (void)__hip_atomic_fetch_add((float*)(U + 2), (float)cro_coh_v_f32(block, tid), RLX, WGRP);
  (void)__hip_atomic_fetch_add((double*)(U + 3), (double)cro_coh_v_f64(g), RLX, WGRP);
  const uint32_t w = cro_coh_v_mm32(g);
  const double x = (double)cro_coh_v_mmf64(g);
  (void)__hip_atomic_fetch_min((uint32_t*)(U + 6), w, RLX, WGRP);
  (void)__hip_atomic_fetch_max((uint32_t*)(U + 7), w, RLX, WGRP);
  (void)__hip_atomic_fetch_min((int32_t*)(U + 8), (int32_t)w, RLX, WGRP);
  (void)__hip_atomic_fetch_max((int32_t*)(U + 9), (int32_t)w, RLX, WGRP);
  (void)__hip_atomic_fetch_min((double*)(U + 10), x, RLX, WGRP);
  (void)__hip_atomic_fetch_max((double*)(U + 11), x, RLX, WGRP);
  (void)__hip_atomic_fetch_and((uint32_t*)(U + 12), cro_coh_v_and32(block, tid, salt), RLX, WGRP);
  (void)__hip_atomic_fetch_or((uint32_t*)(U + 13), cro_coh_v_or32(block, tid, salt), RLX, WGRP);
  (void)__hip_atomic_fetch_xor((uint32_t*)(U + 14), cro_coh_v_xor32(g), RLX, WGRP);
  (void)__hip_atomic_fetch_and(U + 15, cro_coh_v_and64(block, tid, salt), RLX, WGRP);
  (void)__hip_atomic_fetch_or(U + 16, cro_coh_v_or64(block, tid, salt), RLX, WGRP);
  (void)__hip_atomic_fetch_xor(U + 17, cro_coh_v_xor64(g), RLX, WGRP);
}

// What one wave found in one check.  n_bad is wave-uniform (ballot counts);
// first and bits are per lane until reduce().
struct Tally {
  uint32_t n_bad = 0;
  uint32_t first = ~0u;
  uint32_t bits = 0;

  __device__ void add(uint32_t diff, uint32_t where) {
    bits |= diff;
    const unsigned long long mask = __ballot(diff != 0);
    if (mask) {
      n_bad += (uint32_t)__popcll(mask);
      if (diff) first = where < first ? where : first;
    }
  }
  __device__ void add64(uint64_t diff, uint32_t where) {
    add((uint32_t)diff | (uint32_t)(diff >> 32), where);
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

// LDS carve: the unit, the compare-and-swap words, the arrival word's old value
constexpr int kLdsUnit = 0;
constexpr int kLdsCas = CRO_COH_UNIT_WORDS * 8;
constexpr int kLdsOld = kLdsCas + kBlock * 4;

extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

__global__ __launch_bounds__(kBlock) void coherence_kernel(CohParams p) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t block = blockIdx.x, g = block * 256u + tid;
  uint32_t xcc_id, hw_id;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
  const bool inj2 = p.inj_mode == 2 && cro_cov_cu_key(xcc_id, hw_id) == p.inj_key;
  const bool inj1 = p.inj_mode == 1;

  // -- visibility (a): pre-read the group's payloads with plain loads, so this
  // XCD's L2 (and, for a while, this CU's L1) holds the lines that are about
  // to be rewritten; a second pass follows right before the hand-off
  const uint32_t grp0 = block & ~63u;
  const uint32_t n_grp = p.grid - grp0 < 64u ? p.grid - grp0 : 64u;
  uint32_t preread = 0;
  for (uint32_t i = tid; i < n_grp * CRO_COH_PAYLOAD; i += kBlock)
    preread ^= p.payload[(size_t)grp0 * CRO_COH_PAYLOAD + i];

  // -- tallies: the workgroup's own unit, its XCD's, a device-wide one
  {
    const int skip =
        inj2 && p.inj_test < CRO_COH_TALLIES && tid == cro_coh_drop_tid((int)p.inj_test, block)
            ? (int)p.inj_test
            : -1;
    tally_global(p.units + (size_t)block * CRO_COH_UNIT_WORDS, 0, block, tid, p.salt, skip);
    tally_global(p.units + (size_t)cro_coh_xcd_unit(p.grid, xcc_id, block) * CRO_COH_UNIT_WORDS, 1,
                 block, tid, p.salt, skip);
    tally_global(p.units + (size_t)cro_coh_dev_unit(p.grid, block) * CRO_COH_UNIT_WORDS, 1, block,
                 tid, p.salt, skip);
  }

  // -- ticket: every lane draws one and marks it; a ticket beyond the grid is
  // flagged and marks nothing
  Tally t_ticket, t_cas, t_lds;
  {
    const uint32_t n = p.grid * 256u;
    const uint32_t ticket = __hip_atomic_fetch_add(per_lane(p.ticket), 1u, RLX, AGENT);
    const bool beyond = ticket >= n;
    if (!beyond) {
      p.owner[ticket] = g;
      if (!(inj2 && p.inj_test == CRO_COH_TICKET && tid == 0))
        (void)__hip_atomic_fetch_add(p.seen + ticket, 1u, RLX, AGENT);
    }
    t_ticket.add(beyond ? (ticket | 1u) : 0u, g);
  }

  // -- compare-and-swap and exchange on the lane's own line
  {
    uint32_t* line = p.cas + (size_t)g * CRO_COH_CAS_STRIDE;
    uint64_t* line64 = (uint64_t*)(line + 2);
    const uint32_t prev32 = cro_coh_cas32(p.epoch - 1, g), new32 = cro_coh_cas32(p.epoch, g);
    const uint64_t prev64 = cro_coh_cas64(p.epoch - 1, g), new64 = cro_coh_cas64(p.epoch, g);
    uint32_t e32 = prev32;  // must hit: swaps, returns the old value
    (void)__hip_atomic_compare_exchange_strong(line, &e32, new32, RLX, RLX, AGENT);
    uint32_t hit32 = e32;
    e32 = ~new32;  // must miss: leaves memory alone, returns the current value
    (void)__hip_atomic_compare_exchange_strong(line, &e32, 0x0BADC0DEu, RLX, RLX, AGENT);
    const uint32_t miss32 = e32;
    uint64_t e64 = prev64;
    (void)__hip_atomic_compare_exchange_strong(line64, &e64, new64, RLX, RLX, AGENT);
    const uint64_t hit64 = e64;
    e64 = ~new64;
    (void)__hip_atomic_compare_exchange_strong(line64, &e64, 0x0BADC0DE0BADC0DEull, RLX, RLX,
                                               AGENT);
    const uint64_t miss64 = e64;
    const uint32_t xchg = __hip_atomic_exchange(line + 4, cro_coh_xchg32(p.epoch, g), RLX, AGENT);
    uint32_t want_hit32 = prev32;
    if (p.inj_test == CRO_COH_CAS) {
      if (inj2 && tid == 0) hit32 ^= p.inj_flip;
      if (inj1 && lane == 0) want_hit32 ^= p.inj_flip;
    }
    t_cas.add(hit32 ^ want_hit32, 0 * 64 + lane);
    t_cas.add(miss32 ^ new32, 1 * 64 + lane);
    t_cas.add64(hit64 ^ prev64, 2 * 64 + lane);
    t_cas.add64(miss64 ^ new64, 3 * 64 + lane);
    t_cas.add(xchg ^ cro_coh_xchg32(p.epoch - 1, g), 4 * 64 + lane);
  }

  // -- LDS read-modify-write: four waves contend on one unit
  {
    uint64_t* unit = (uint64_t*)(smem + kLdsUnit);
    uint32_t* lcas = (uint32_t*)(smem + kLdsCas);
    if (tid < CRO_COH_UNIT_WORDS) unit[tid] = p.init_unit[tid];
    lcas[tid] = g * 3u + 1u;
    __syncthreads();
    tally_lds(unit, block, tid, p.salt);
    uint32_t e = g * 3u + 1u;
    (void)__hip_atomic_compare_exchange_strong(per_lane(lcas) + tid, &e, ~g, RLX, RLX, WGRP);
    __syncthreads();
    if (inj2 && p.inj_test == CRO_COH_LDS && tid == 0) unit[0] ^= p.inj_flip;
    __syncthreads();
    t_lds.add(e ^ (g * 3u + 1u), 32 + tid);
    t_lds.add(lcas[tid] ^ ~g, 32 + tid);
    if (wave == 0) {
      const bool slot =
          lane < CRO_COH_SLOTS && lane != CRO_COH_PK_F16 && lane != CRO_COH_PK_BF16;
      const uint64_t got = slot ? unit[lane] : 0;
      const uint64_t want =
          slot ? p.expect_wg[(size_t)block * CRO_COH_UNIT_WORDS + lane] : 0;
      t_lds.add64(got ^ want, lane);
    }
  }

  // -- visibility (a) again, right before the hand-off: after the work above
  // the first pass's lines need no longer be in L1, and a consumer whose L1
  // is cold cannot see a missing invalidate
  __syncthreads();
  for (uint32_t i = tid; i < n_grp * CRO_COH_PAYLOAD; i += kBlock)
    preread ^= p.payload[(size_t)grp0 * CRO_COH_PAYLOAD + i];

  // -- visibility (b): store the payload with plain stores and publish it by
  // the valid producer form: every storing wave drains, a barrier, lane 0
  // releases at agent scope, waits again and sets the workgroup's arrival bit
  if (lane < 16) {
    const uint32_t idx = wave * 16 + lane;
    uint32_t v = cro_coh_payload(p.seed, p.epoch, block, idx);
    if (inj2 && p.inj_test == CRO_COH_VIS && idx == 5) v ^= p.inj_flip;
    p.payload[(size_t)block * CRO_COH_PAYLOAD + idx] = v;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  uint64_t* lds_old = (uint64_t*)(smem + kLdsOld);
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint64_t old =
        __hip_atomic_fetch_or(p.words + (block >> 6), 1ull << (block & 63u), RLX, AGENT);
    *lds_old = old;
    // -- (c) the consumer form: one agent acquire, a wait, the barrier, plain loads
    if (p.inj_mode != 3) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  uint64_t old = *lds_old;
  // (the builtin returns int: without the casts a set bit 31 would sign-extend)
  old = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(old >> 32)) << 32) |
        (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)old);
  // only blocks of this group exist: a bit beyond them is a wrong value
  // returned, never an address
  const uint64_t exist = n_grp == 64 ? ~0ull : ((1ull << n_grp) - 1ull);
  Tally t_vis;
  uint32_t vis_pairs = 0, vis_stale = 0;
  if (wave == 0) t_vis.add64(lane == 0 ? (old & ~exist) : 0, (grp0 + 63u) * 64u);
  for (uint64_t m = old & exist; m; m &= m - 1) {
    const uint32_t bit = (uint32_t)__builtin_ctzll(m);
    if ((bit & 3u) != wave) continue;
    const uint32_t prod = grp0 + bit;
    const uint32_t got = p.payload[(size_t)prod * CRO_COH_PAYLOAD + lane];
    uint32_t want = cro_coh_payload(p.seed, p.epoch, prod, lane);
    if (inj1 && p.inj_test == CRO_COH_VIS && lane == 0) want ^= p.inj_flip;
    const uint32_t diff = got ^ want;
    vis_stale += (uint32_t)__popcll(
        __ballot(diff != 0 && got == cro_coh_payload(p.seed, p.epoch - 1, prod, lane)));
    t_vis.add(diff, prod * 64u + lane);
    ++vis_pairs;
  }

  t_ticket.reduce();
  t_cas.reduce();
  t_lds.reduce();
  t_vis.reduce();
  for (int off = 32; off > 0; off >>= 1) preread ^= __shfl_xor(preread, off, 64);
  if (lane == 0) {
    CroCoherenceRecord rec;
    rec.xcc_id = xcc_id;
    rec.hw_id = hw_id;
    rec.fail_mask = (t_ticket.n_bad ? 1u << CRO_COH_TICKET : 0u) |
                    (t_cas.n_bad ? 1u << CRO_COH_CAS : 0u) |
                    (t_lds.n_bad ? 1u << CRO_COH_LDS : 0u) |
                    (t_vis.n_bad ? 1u << CRO_COH_VIS : 0u);
    const Tally& lead = t_ticket.n_bad ? t_ticket : t_cas.n_bad ? t_cas : t_lds.n_bad ? t_lds : t_vis;
    rec.n_bad = lead.n_bad;
    rec.first_bad = lead.first;
    rec.bits_bad = lead.bits;
    rec.valid = 1;
    rec.block = block;
    rec.vis_pairs = vis_pairs;
    rec.vis_bad = t_vis.n_bad;
    rec.vis_stale = vis_stale;
    rec.vis_first_block = t_vis.n_bad ? t_vis.first >> 6 : ~0u;
    rec.vis_first_dword = t_vis.n_bad ? t_vis.first & 63u : ~0u;
    rec.vis_bits = t_vis.bits;
    rec.preread = preread;
    rec.epoch = p.epoch;
    p.records[block * kWaves + wave] = rec;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// Per-device cached context (CtxBase, crohost.h); the buffers grow on demand
// with the grid and the epochs of a round.
struct CohCtx : CtxBase {
  int cus = 0;
  int cap_grid = 0, cap_iters = 0;
  uint64_t* d_units = nullptr;
  uint32_t* d_ticket = nullptr;
  uint32_t* d_seen = nullptr;
  uint32_t* d_owner = nullptr;
  uint32_t* d_cas = nullptr;
  uint32_t* d_payload = nullptr;
  uint64_t* d_words = nullptr;
  uint64_t* d_expect = nullptr;
  uint64_t* d_init = nullptr;
  CroCoherenceRecord* d_records = nullptr;
};
CohCtx g_cctx[kMaxDevices];

constexpr int kTicketStride = 32;  // dwords: every epoch's counter on a line of its own
constexpr int kWordsPerEpoch = CRO_COH_MAX_GRID / CRO_COH_GROUP;

int prepare(CohCtx* ctx, int device, int grid, int iters, CroCoherenceResult* out) {
  if (!ctx->ready) {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, device));
    ctx->cus = prop.multiProcessorCount;
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(coherence_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               CRO_COV_MAX_LDS_BYTES));
    CHECK(hipEventCreate(&ctx->e0));
    CHECK(hipEventCreate(&ctx->e1));
    CHECK(hipMalloc(&ctx->d_init, CRO_COH_UNIT_WORDS * 8));
    ctx->ready = 1;
  }
  if (grid == 0) grid = ctx->cus;
  if (grid <= ctx->cap_grid && iters <= ctx->cap_iters) return 0;
  for (void* q : {(void*)ctx->d_units, (void*)ctx->d_ticket, (void*)ctx->d_seen,
                  (void*)ctx->d_owner, (void*)ctx->d_cas, (void*)ctx->d_payload,
                  (void*)ctx->d_words, (void*)ctx->d_expect, (void*)ctx->d_records})
    if (q) (void)hipFree(q);
  ctx->cap_grid = ctx->cap_iters = 0;
  ctx->d_units = ctx->d_words = ctx->d_expect = nullptr;
  ctx->d_ticket = ctx->d_seen = ctx->d_owner = ctx->d_cas = ctx->d_payload = nullptr;
  ctx->d_records = nullptr;
  const size_t g = (size_t)(grid > ctx->cap_grid ? grid : ctx->cap_grid);
  const size_t e = (size_t)(iters > ctx->cap_iters ? iters : ctx->cap_iters);
  const size_t lanes = g * 256;
  CHECK(hipMalloc(&ctx->d_units, e * cro_coh_units((int)g) * CRO_COH_UNIT_WORDS * 8));
  CHECK(hipMalloc(&ctx->d_ticket, e * kTicketStride * 4));
  CHECK(hipMalloc(&ctx->d_seen, e * lanes * 4));
  CHECK(hipMalloc(&ctx->d_owner, e * lanes * 4));
  CHECK(hipMalloc(&ctx->d_cas, lanes * CRO_COH_CAS_STRIDE * 4));
  CHECK(hipMalloc(&ctx->d_payload, g * CRO_COH_PAYLOAD * 4));
  CHECK(hipMalloc(&ctx->d_words, e * kWordsPerEpoch * 8));
  CHECK(hipMalloc(&ctx->d_expect, e * g * CRO_COH_UNIT_WORDS * 8));
  CHECK(hipMalloc(&ctx->d_records, e * g * kWaves * sizeof(CroCoherenceRecord)));
  ctx->cap_grid = (int)g;
  ctx->cap_iters = (int)e;
  return 0;
}

// first slot of a tally check in a unit
int first_slot(int test) { return test < 6 ? test : test == CRO_COH_MINMAX ? 6 : 12; }

void describe(const CroCoherenceAgg& a, CroCoherenceResult* out) {
  static const char* const kLevel[] = {"workgroup", "xcd", "device"};
  const int test = __builtin_ctz(a.fail_mask);
  if (test < CRO_COH_TALLIES && a.tally_level >= 0) {
    snprintf(out->msg, sizeof(out->msg),
             "coherence mismatch in %s: %s line %d slot %d epoch %d got 0x%016llx want "
             "0x%016llx at xcd=%d se=%d sh=%d cu=%d; %llu slots bad",
             out->failed_test, kLevel[a.tally_level], a.tally_unit, a.tally_slot, a.tally_epoch,
             a.tally_got, a.tally_want, a.xcd, a.se, a.sh, a.cu, a.bad[test]);
  } else if (test == CRO_COH_TICKET && a.first_bad_index < 0) {
    snprintf(out->msg, sizeof(out->msg),
             "coherence mismatch in ticket: slot %d epoch %d marked %u times, drawn by lane %u "
             "at xcd=%d se=%d sh=%d cu=%d simd=%d; %llu slots bad",
             a.ticket_slot, a.ticket_epoch, a.ticket_seen, a.ticket_owner, a.xcd, a.se, a.sh,
             a.cu, a.simd, a.bad[test]);
  } else if (a.first_bad_index >= 0) {
    snprintf(out->msg, sizeof(out->msg),
             "coherence mismatch in %s at xcd=%d se=%d sh=%d cu=%d simd=%d: first %u, bits "
             "0x%08x, block %d; %llu of %llu waves bad on %d CUs; visibility %llu bad %llu stale",
             out->failed_test, a.xcd, a.se, a.sh, a.cu, a.simd, a.first_bad, a.bits_bad,
             a.bad_block, a.waves_bad, a.waves_run, a.cus_bad, a.vis_bad, a.vis_stale);
  } else {
    snprintf(out->msg, sizeof(out->msg),
             "coherence mismatch in %s: %llu of %llu pairs checked, %llu arrival counts or words "
             "wrong",
             out->failed_test, a.pairs_checked, a.pairs_expected, a.bad[test]);
  }
}

int run_coherence(int device, const CroCoherenceOpts* opts, CroCoherenceResult* out,
                  CroCoherenceRecord* records_out, int max_records, unsigned long long* units_out,
                  long long max_unit_words) {
  CroCoherenceOpts o;
  memset(&o, 0, sizeof(o));
  if (opts) o = *opts;
  if (o.grid_blocks < 0 || o.grid_blocks > CRO_COH_MAX_GRID) return bad_arg(out, "grid_blocks");
  if (o.iters < 0 || o.iters > CRO_COH_MAX_ITERS) return bad_arg(out, "iters");
  if (o.max_rounds < 0 || o.max_rounds > kMaxRounds) return bad_arg(out, "max_rounds");
  if (!(o.min_cu_fraction >= 0.0 && o.min_cu_fraction <= 1.0))
    return bad_arg(out, "min_cu_fraction");
  if (o.selftest_mode < 0 || o.selftest_mode > 3) return bad_arg(out, "selftest_mode");
  if (o.selftest_mode == 1 || o.selftest_mode == 2) {
    if (o.selftest_test < 0 || o.selftest_test >= CRO_COH_TESTS)
      return bad_arg(out, "selftest_test");
    if (o.selftest_bit < 0 || o.selftest_bit > 31) return bad_arg(out, "selftest_bit");
  }
  const int iters = o.iters ? o.iters : kDefaultIters;
  const int max_rounds = o.max_rounds ? o.max_rounds : kDefaultRounds;

  std::unique_lock<std::mutex> lock;
  CohCtx* ctx = enter_device(g_cctx, device, lock, out->msg, sizeof(out->msg));
  if (ctx == nullptr) return -1;
  if (prepare(ctx, device, o.grid_blocks, iters, out) != 0) return -1;
  const int grid = o.grid_blocks ? o.grid_blocks : ctx->cus;
  if (grid < 1 || grid > CRO_COH_MAX_GRID) return bad_arg(out, "device compute units");
  out->cus_expected = ctx->cus;
  out->grid_blocks = grid;
  out->iters = iters;

  const size_t lanes = (size_t)grid * 256;
  const size_t units = (size_t)cro_coh_units(grid);
  const size_t unit_words = units * CRO_COH_UNIT_WORDS;  // per epoch
  const size_t per_launch = (size_t)grid * kWaves;
  const uint32_t flip = 1u << (o.selftest_bit & 31);

  // what does not depend on the round: the initial images and the expected
  // workgroup units of every epoch (no placement enters those)
  std::vector<uint64_t> h_init(unit_words * iters), h_expect((size_t)grid * CRO_COH_UNIT_WORDS * iters);
  std::vector<uint32_t> h_payload((size_t)grid * CRO_COH_PAYLOAD);
  for (int e = 0; e < iters; ++e) {
    cro_coh_initial_units(grid, h_init.data() + e * unit_words);
    const uint32_t salt = cro_coh_salt(o.seed, (uint32_t)e + 1);
    for (int b = 0; b < grid; ++b) {
      CroCohTotals t;
      cro_coh_block_totals((uint32_t)b, salt, 0, &t);
      cro_coh_encode(&t, h_expect.data() + ((size_t)e * grid + b) * CRO_COH_UNIT_WORDS);
    }
  }
  if (o.selftest_mode == 1 && o.selftest_test == CRO_COH_LDS) h_expect[0] ^= flip;
  for (size_t i = 0; i < h_payload.size(); ++i)
    h_payload[i] = cro_coh_payload(o.seed, 0, (uint32_t)(i / CRO_COH_PAYLOAD),
                                   (uint32_t)(i % CRO_COH_PAYLOAD));
  CHECK(hipMemcpy(ctx->d_init, h_init.data(), CRO_COH_UNIT_WORDS * 8, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(ctx->d_expect, h_expect.data(), h_expect.size() * 8, hipMemcpyHostToDevice));

  std::vector<CroCoherenceRecord> records;
  std::vector<uint64_t> got(unit_words * iters), want(unit_words);
  std::vector<uint32_t> seen(lanes * iters), owner(lanes * iters), xcc_of(grid);
  std::vector<uint64_t> words((size_t)kWordsPerEpoch * iters);
  CroCoherenceAgg host;  // what the host's own comparisons found, over all rounds
  cro_coherence_agg_clear(&host);
  int rounds = 0;
  double gpu_ms = 0.0;
  for (;;) {
    // fresh buffers for this round's epochs
    CHECK(hipMemcpy(ctx->d_units, h_init.data(), h_init.size() * 8, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(ctx->d_payload, h_payload.data(), h_payload.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(ctx->d_ticket, 0, (size_t)iters * kTicketStride * 4));
    CHECK(hipMemset(ctx->d_seen, 0, lanes * iters * 4));
    CHECK(hipMemset(ctx->d_owner, 0xFF, lanes * iters * 4));
    CHECK(hipMemset(ctx->d_cas, 0, lanes * CRO_COH_CAS_STRIDE * 4));
    CHECK(hipMemset(ctx->d_words, 0, (size_t)iters * kWordsPerEpoch * 8));
    CHECK(hipMemset(ctx->d_records, 0, per_launch * iters * sizeof(CroCoherenceRecord)));
    CHECK(hipDeviceSynchronize());
    const auto one_round = [&] {
      for (int e = 0; e < iters; ++e) {
        CohParams p;
        memset(&p, 0, sizeof(p));
        p.units = ctx->d_units + e * unit_words;
        p.ticket = ctx->d_ticket + (size_t)e * kTicketStride;
        p.seen = ctx->d_seen + e * lanes;
        p.owner = ctx->d_owner + e * lanes;
        p.cas = ctx->d_cas;
        p.payload = ctx->d_payload;
        p.words = ctx->d_words + (size_t)e * kWordsPerEpoch;
        p.expect_wg = ctx->d_expect + (size_t)e * grid * CRO_COH_UNIT_WORDS;
        p.init_unit = ctx->d_init;
        p.records = ctx->d_records + e * per_launch;
        p.grid = (uint32_t)grid;
        p.epoch = (uint32_t)e + 1;
        p.seed = o.seed;
        p.salt = cro_coh_salt(o.seed, p.epoch);
        p.inj_mode = (uint32_t)o.selftest_mode;
        p.inj_test = (uint32_t)o.selftest_test;
        p.inj_key = o.selftest_key;
        p.inj_flip = flip;
        hipLaunchKernelGGL(coherence_kernel, dim3(grid), dim3(kBlock),
                           (size_t)CRO_COV_MAX_LDS_BYTES, 0, p);
      }
    };
    float ms = 0.f;
    CHECK(timed_ms(*ctx, &ms, one_round));
    gpu_ms += ms;
    records.resize((size_t)(rounds + 1) * iters * per_launch);
    CroCoherenceRecord* round_records = records.data() + (size_t)rounds * iters * per_launch;
    CHECK(hipMemcpy(round_records, ctx->d_records,
                     per_launch * iters * sizeof(CroCoherenceRecord), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(got.data(), ctx->d_units, got.size() * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(seen.data(), ctx->d_seen, seen.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(owner.data(), ctx->d_owner, owner.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(words.data(), ctx->d_words, words.size() * 8, hipMemcpyDeviceToHost));
    ++rounds;
    cro_coherence_aggregate(records.data(), grid, rounds * iters, &out->agg);
    if (out->agg.waves_run == (unsigned long long)records.size()) {
      for (int e = 0; e < iters; ++e) {
        const CroCoherenceRecord* lr = round_records + e * per_launch;
        for (int b = 0; b < grid; ++b) xcc_of[b] = lr[(size_t)b * kWaves].xcc_id;
        cro_coh_expected_units(grid, o.seed, (uint32_t)e + 1, xcc_of.data(), want.data());
        if (o.selftest_mode == 1 && o.selftest_test < CRO_COH_TALLIES && e == 0)
          want[first_slot(o.selftest_test)] ^= flip;
        cro_coh_check_tallies(got.data() + e * unit_words, want.data(), grid, e + 1, lr, &host);
        const uint32_t want_of_0 =
            o.selftest_mode == 1 && o.selftest_test == CRO_COH_TICKET && e == 0 ? 1u ^ flip : 1u;
        cro_coh_check_tickets(seen.data() + e * lanes, owner.data() + e * lanes, grid, e + 1,
                              want_of_0, lr, &host);
        cro_coh_check_words(words.data() + (size_t)e * kWordsPerEpoch, grid, &host);
      }
    }
    cro_coh_agg_merge(&out->agg, &host);
    if (out->agg.fail_mask || out->agg.waves_run != (unsigned long long)records.size() ||
        out->agg.cus_seen >= ctx->cus || rounds >= max_rounds)
      break;
  }
  out->rounds = rounds;
  out->gpu_ms = gpu_ms;
  const size_t n_last = (size_t)iters * per_launch;
  if (records_out && max_records > 0) {
    const size_t m = n_last < (size_t)max_records ? n_last : (size_t)max_records;
    memcpy(records_out, records.data() + (size_t)(rounds - 1) * n_last,
           m * sizeof(CroCoherenceRecord));
  }
  if (units_out && max_unit_words > 0) {
    const size_t m = got.size() < (size_t)max_unit_words ? got.size() : (size_t)max_unit_words;
    memcpy(units_out, got.data(), m * 8);
  }
  const CroCoherenceAgg& a = out->agg;
  if (a.waves_run != records.size()) {
    // a wave that never wrote its record: the launch did not run to the end
    snprintf(out->msg, sizeof(out->msg), "%llu of %zu waves reported", a.waves_run,
             records.size());
    return -1;
  }
  if (a.fail_mask) {
    if (a.first_bad_index >= 0) {
      out->first_bad_round = (int)((size_t)a.first_bad_index / n_last);
      out->first_bad_record = (int)((size_t)a.first_bad_index % n_last);
    }
    snprintf(out->failed_test, sizeof(out->failed_test), "%s", cro_coh_test_name(a.fail_mask));
    describe(a, out);
    return -34;
  }
  if (o.min_cu_fraction > 0.0 && (double)a.cus_seen < o.min_cu_fraction * (double)ctx->cus) {
    snprintf(out->msg, sizeof(out->msg),
             "coverage %d of %d CUs after %d rounds is below the floor %.3f", a.cus_seen,
             ctx->cus, rounds, o.min_cu_fraction);
    return -35;
  }
  out->ok = 1;
  snprintf(out->msg, sizeof(out->msg), "ok");
  return 0;
}

}  // namespace

extern "C" int cro_coherence_run_records(int device, const struct CroCoherenceOpts* opts,
                                         struct CroCoherenceResult* out,
                                         struct CroCoherenceRecord* records_out, int max_records,
                                         unsigned long long* units_out,
                                         long long max_unit_words) {
  memset(out, 0, sizeof(*out));
  out->first_bad_round = out->first_bad_record = -1;
  cro_coherence_agg_clear(&out->agg);
  const double t0 = now_ms();
  out->rc = run_coherence(device, opts, out, records_out, max_records, units_out, max_unit_words);
  out->t_total_ms = now_ms() - t0;
  return out->rc;
}

extern "C" int cro_coherence_run(int device, const struct CroCoherenceOpts* opts,
                                 struct CroCoherenceResult* out) {
  return cro_coherence_run_records(device, opts, out, nullptr, 0, nullptr, 0);
}
