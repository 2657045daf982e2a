// cro_amd gfx950 LDS scrub stage: clear and verify every CU's LDS before a
// device is drained (croldsscrub.h says what that covers and what it does not).
//
// One kernel, one 256-thread workgroup per CU: the dynamic-LDS request is
// always a CU's whole 160 KiB, which is what places one workgroup per CU
// (coverage.hip, profiles/compute_probe_mi355x.md).  Each workgroup, on the
// first lds_bytes of its LDS, with 16-byte accesses only:
//
//   census — load every word as found and count those that differ from the
//            fill word, before this kernel stores anything;
//   fill   — store the fill word to every word;
//   verify — load every word back, each thread the vectors that its mirror
//            thread (255 - t) filled, so a pass shows that the data went
//            through LDS and not through a register.
//
// Counts are reduced per wave with 64-lane ballots, 64-bit popcounts and
// shuffles, never through LDS (scratch there would be residue of our own), and
// a wave adds to its workgroup's record in global memory only when it has
// something to add.  Workgroups are independent: no inter-workgroup
// communication, no spin, no grid barrier.  The host aggregates the records
// (croldsscrub.h), launches the same grid again, a bounded number of times,
// while some CU is still unseen, and ends with a census-only dispatch.
//
// A library of its own, libcroldsscrub.so (cro_amd/hip/build.py:
// build_lds_scrub); host plumbing shared with the other stages in crohost.h.

#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>

#include "crohost.h"
#include "croldsscrub.h"

namespace {

constexpr uint32_t kLdsVecs = CRO_LDS_SCRUB_BYTES / 16;
static_assert(kLdsVecs % kBlock == 0, "every trip of the march is a whole workgroup wide");
constexpr int kDefaultRounds = 4;  // the bounds of the coverage stage
constexpr int kMaxRounds = 64;
constexpr int kMaxGrid = 1 << 16;

// ---------------------------------------------------------------------------
// kernel
// ---------------------------------------------------------------------------

struct LdsParams {
  CroLdsScrubRecord* records;  // this dispatch's `grid` records
  uint32_t n4;                 // 16-byte vectors marched
  uint32_t fill_word;
  uint32_t census_only;
  uint32_t mode;  // self-test, see croldsscrub.h
  uint32_t pattern;
  uint32_t st_word;
  uint32_t st_flip;  // 1 << selftest_bit
};

// What one wave found in one phase.  n is wave-uniform (ballot counts); first
// and bits are per lane until reduce().
struct Tally {
  uint32_t n = 0;
  uint32_t first = ~0u;
  uint32_t bits = 0;

  // every lane of the wave calls it
  __device__ void add(uint32_t diff, uint32_t word) {
    bits |= diff;
    const unsigned long long mask = __ballot(diff != 0);
    if (mask) {
      n += (uint32_t)__popcll(mask);
      if (diff) first = word < first ? word : first;
    }
  }
  __device__ void add(uint4 got, uint32_t want, uint32_t vec) {
    add(got.x ^ want, (vec << 2) + 0);
    add(got.y ^ want, (vec << 2) + 1);
    add(got.z ^ want, (vec << 2) + 2);
    add(got.w ^ want, (vec << 2) + 3);
  }
  // every lane of the wave calls it (n is uniform, so the branch is)
  __device__ void reduce() {
    if (!n) return;
    for (int off = 32; off > 0; off >>= 1) {
      bits |= __shfl_xor(bits, off, 64);
      const uint32_t other = __shfl_xor(first, off, 64);
      first = other < first ? other : first;
    }
  }
};

__device__ inline uint4 splat(uint32_t w) { return make_uint4(w, w, w, w); }

__device__ inline void set_word(uint4& v, uint32_t j, uint32_t w) {
  if (j == 0) v.x = w;
  if (j == 1) v.y = w;
  if (j == 2) v.z = w;
  if (j == 3) v.w = w;
}

// Who touches vector v (slot s = v % 256):
//   census, fill, guard check   thread s
//   verify                      thread 255 - s
//   self-test stores            thread s ^ 64
// The three differ for every s, so no thread ever loads a word that it
// stored itself except where the fill follows the same thread's census.
// Every loop runs on its wave's base index, which the 64 lanes share, so all
// of them reach every ballot; lanes past the end compare equal.
__global__ __launch_bounds__(kBlock) void lds_scrub_kernel(LdsParams p) {
  // all LDS is dynamic, so its base stays 16-byte aligned for the b128 accesses
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* lds4 = reinterpret_cast<uint4*>(smem);

  const uint32_t tid = threadIdx.x, lane = tid & 63;
  uint32_t xcc_id, hw_id;  // for the report only
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
  CroLdsScrubRecord* rec = p.records + blockIdx.x;
  const uint32_t n4 = p.n4;
  const uint4 fill = splat(p.fill_word);
  const uint32_t st_vec = p.st_word >> 2;

  if (p.mode) {  // self-test plant, and the guard over what is not marched
    const uint32_t body = p.mode == 2 ? p.fill_word : p.pattern;
    for (uint32_t v = tid ^ 64; v < kLdsVecs; v += kBlock) {
      if (v >= n4) {
        lds4[v] = splat(CRO_LDS_SCRUB_GUARD_WORD);
      } else if (p.mode != 4) {
        uint4 x = splat(body);
        if (p.mode == 2 && v == st_vec) set_word(x, p.st_word & 3, p.pattern);
        lds4[v] = x;
      }
    }
    __syncthreads();
  }

  Tally census;
  for (uint32_t v0 = tid - lane; v0 < n4; v0 += kBlock) {
    const uint32_t v = v0 + lane;
    uint4 got = fill;
    if (v < n4) got = lds4[v];
    census.add(got, p.fill_word, v);
  }
  census.reduce();
  if (census.n && lane == 0) {
    atomicAdd(&rec->dirty_words, census.n);
    atomicMin(&rec->first_dirty, census.first);
  }

  if (!p.census_only) {
    __syncthreads();
    if (p.mode != 3)
      for (uint32_t v = tid; v < n4; v += kBlock) lds4[v] = fill;
    __syncthreads();
    if (p.mode == 4) {
      if (tid == ((st_vec & (kBlock - 1)) ^ 64)) {
        uint4 x = lds4[st_vec], flip = splat(0);
        set_word(flip, p.st_word & 3, p.st_flip);
        lds4[st_vec] = make_uint4(x.x ^ flip.x, x.y ^ flip.y, x.z ^ flip.z, x.w ^ flip.w);
      }
      __syncthreads();
    }

    Tally verify;
    for (uint32_t v0 = (kBlock - 64) - (tid - lane); v0 < n4; v0 += kBlock) {
      const uint32_t v = v0 + (63 - lane);  // slot 255 - tid
      uint4 got = fill;
      if (v < n4) got = lds4[v];
      verify.add(got, p.fill_word, v);
    }
    verify.reduce();
    if (verify.n && lane == 0) {
      atomicAdd(&rec->n_bad, verify.n);
      atomicMin(&rec->first_bad, verify.first);
      atomicOr(&rec->bits_bad, verify.bits);
    }

    if (p.mode) {
      Tally guard;
      for (uint32_t v0 = tid - lane; v0 < kLdsVecs; v0 += kBlock) {
        const uint32_t v = v0 + lane;  // below kLdsVecs: whole trips
        uint4 got = splat(CRO_LDS_SCRUB_GUARD_WORD);
        if (v >= n4) {
          got = lds4[v];
          lds4[v] = fill;  // counted; the self-test leaves no guard words behind
        }
        guard.add(got, CRO_LDS_SCRUB_GUARD_WORD, v);
      }
      if (guard.n && lane == 0) atomicAdd(&rec->guard_bad, guard.n);
    }
  }

  if (tid == 0) {
    rec->xcc_id = xcc_id;
    rec->hw_id = hw_id;
    rec->valid = 1;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// Per-device cached context (CtxBase, crohost.h): the events and the record
// buffer, which grows on demand.
struct LdsCtx : CtxBase {
  int cus = 0;
  CroLdsScrubRecord* d_records = nullptr;
  size_t records_cap = 0;
};
LdsCtx g_lctx[kMaxDevices];

int run_lds_scrub(int device, const CroLdsScrubOpts* opts, CroLdsScrubResult* out,
                  CroLdsScrubRecord* records_out, int max_records) {
  CroLdsScrubOpts o;
  memset(&o, 0, sizeof(o));
  if (opts) o = *opts;
  if (o.grid < 0 || o.grid > kMaxGrid) return bad_arg(out, "grid");
  if (o.lds_bytes < 0 || o.lds_bytes > CRO_LDS_SCRUB_BYTES || (o.lds_bytes & 15))
    return bad_arg(out, "lds_bytes must be a multiple of 16, at most 163840");
  if (o.max_rounds < 0 || o.max_rounds > kMaxRounds) return bad_arg(out, "max_rounds");
  if (!(o.min_cu_fraction >= 0.0 && o.min_cu_fraction <= 1.0))  // refuses a NaN too
    return bad_arg(out, "min_cu_fraction");
  const int lds_bytes = o.lds_bytes ? o.lds_bytes : CRO_LDS_SCRUB_BYTES;
  const int max_rounds = o.max_rounds ? o.max_rounds : kDefaultRounds;
  if (o.selftest_mode < 0 || o.selftest_mode > 4) return bad_arg(out, "selftest_mode");
  if (o.selftest_mode) {
    if (o.fill_word == CRO_LDS_SCRUB_GUARD_WORD)
      return bad_arg(out, "fill_word equals the self-test guard word");
    if (o.selftest_pattern == CRO_LDS_SCRUB_GUARD_WORD)
      return bad_arg(out, "selftest_pattern equals the self-test guard word");
    if (o.selftest_pattern == o.fill_word)
      return bad_arg(out, "selftest_pattern equals fill_word");
    if (o.selftest_bit < 0 || o.selftest_bit > 31) return bad_arg(out, "selftest_bit");
    if (o.selftest_word >= (unsigned)lds_bytes / 4) return bad_arg(out, "selftest_word");
  }

  std::unique_lock<std::mutex> lock;
  LdsCtx* ctx = enter_device(g_lctx, device, lock, out->msg, sizeof(out->msg));
  if (ctx == nullptr) return -1;
  if (!ctx->ready) {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, device));
    ctx->cus = prop.multiProcessorCount;
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(lds_scrub_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, CRO_LDS_SCRUB_BYTES));
    CHECK(hipEventCreate(&ctx->e0));
    CHECK(hipEventCreate(&ctx->e1));
    ctx->ready = 1;
  }
  const int grid = o.grid ? o.grid : ctx->cus;
  if (grid < 1) return bad_arg(out, "device reports no compute units");
  // the rounds' records, then the recheck's
  const size_t n_rounds_max = (size_t)grid * (size_t)max_rounds;
  const size_t n_max = n_rounds_max + (size_t)grid;
  if (ctx->records_cap < n_max) {
    if (ctx->d_records) (void)hipFree(ctx->d_records);
    ctx->d_records = nullptr;
    ctx->records_cap = 0;
    CHECK(hipMalloc(&ctx->d_records, n_max * sizeof(CroLdsScrubRecord)));
    ctx->records_cap = n_max;
  }
  out->cus_expected = ctx->cus;
  out->grid = grid;
  out->lds_bytes = lds_bytes;

  const CroLdsScrubRecord clean = CRO_LDS_SCRUB_CLEAN_RECORD;
  std::vector<CroLdsScrubRecord> records(n_max, clean);
  CHECK(hipMemcpy(ctx->d_records, records.data(), n_max * sizeof(clean), hipMemcpyHostToDevice));

  LdsParams p;
  p.n4 = (uint32_t)lds_bytes / 16;
  p.fill_word = o.fill_word;
  p.census_only = 0;
  p.mode = (uint32_t)o.selftest_mode;
  p.pattern = o.selftest_pattern;
  p.st_word = o.selftest_word;
  p.st_flip = 1u << (o.selftest_bit & 31);
  // one dispatch into the records from `first`, event-timed and copied back
  const auto dispatch = [&](size_t first) -> hipError_t {
    p.records = ctx->d_records + first;
    float ms = 0.f;
    TRY(timed_ms(*ctx, &ms, [&] {
      hipLaunchKernelGGL(lds_scrub_kernel, dim3(grid), dim3(kBlock), CRO_LDS_SCRUB_BYTES, 0, p);
    }));
    out->gpu_ms += ms;
    return hipMemcpy(records.data() + first, p.records, (size_t)grid * sizeof(clean),
                     hipMemcpyDeviceToHost);
  };

  CroLdsScrubAgg agg;
  int rounds = 0;
  do {
    CHECK(dispatch((size_t)rounds * grid));
    ++rounds;
    cro_lds_scrub_aggregate(records.data(), (size_t)rounds * grid, &agg);
  } while (agg.cus_seen < ctx->cus && rounds < max_rounds);
  const size_t n = (size_t)rounds * grid;
  if (records_out && max_records > 0) {
    const size_t m = n < (size_t)max_records ? n : (size_t)max_records;
    memcpy(records_out, records.data(), m * sizeof(clean));
  }
  out->rounds = rounds;
  out->cus_seen = agg.cus_seen;
  out->xcds_seen = agg.xcds_seen;
  out->workgroups = agg.workgroups;
  out->bytes_scrubbed = o.selftest_mode == 3 ? 0ull : agg.workgroups * (unsigned long long)lds_bytes;
  out->dirty_words_before = agg.dirty_words;
  out->dirty_workgroups = agg.dirty_workgroups;
  out->first_dirty_word = agg.first_dirty_word;
  out->n_bad = agg.n_bad;
  out->guard_bad = agg.guard_bad;
  out->bad_workgroups = (int)agg.bad_workgroups;
  out->first_bad_word = agg.first_bad_word;
  out->bits_bad = agg.bits_bad;
  out->xcd = agg.xcd;
  out->se = agg.se;
  out->sh = agg.sh;
  out->cu = agg.cu;
  if (agg.workgroups != n) {
    // a workgroup that never wrote its record: the launch did not run to the end
    snprintf(out->msg, sizeof(out->msg), "%llu of %zu workgroups reported", agg.workgroups, n);
    return -1;
  }

  // -- recheck: what a later dispatch, and so the next tenant, would find -------
  if (!o.skip_recheck) {
    p.census_only = 1;
    p.mode = 0;
    CHECK(dispatch(n_rounds_max));
    CroLdsScrubAgg re;
    cro_lds_scrub_aggregate(records.data() + n_rounds_max, (size_t)grid, &re);
    if (re.workgroups != (size_t)grid) {
      snprintf(out->msg, sizeof(out->msg), "%llu of %d recheck workgroups reported",
               re.workgroups, grid);
      return -1;
    }
    out->recheck_dirty_words = re.dirty_words;
    if (re.dirty_words && !agg.n_bad) {
      // nothing was bad in the rounds: the first dirty recheck workgroup leads
      for (size_t i = n_rounds_max; i < n_max; ++i) {
        const CroLdsScrubRecord& r = records[i];
        if (!r.dirty_words) continue;
        const CroCoverageLoc loc = cro_cov_decode(r.xcc_id, r.hw_id);
        out->xcd = (int)loc.xcd;
        out->se = (int)loc.se;
        out->sh = (int)loc.sh;
        out->cu = (int)loc.cu;
        out->first_bad_word = r.first_dirty;
        break;
      }
    }
  }

  // -- gates -------------------------------------------------------------------
  if (out->n_bad || out->recheck_dirty_words) {
    snprintf(out->msg, sizeof(out->msg),
             "LDS residue at xcd=%d se=%d sh=%d cu=%d: first_bad_word %u, bits 0x%08x; "
             "%llu bad words in %d workgroups, %llu dirty at the recheck, %llu guard words "
             "changed",
             out->xcd, out->se, out->sh, out->cu, out->first_bad_word, out->bits_bad,
             out->n_bad, out->bad_workgroups, out->recheck_dirty_words, out->guard_bad);
    return -42;
  }
  if (o.min_cu_fraction > 0.0 &&
      (double)out->cus_seen < o.min_cu_fraction * (double)ctx->cus) {
    snprintf(out->msg, sizeof(out->msg),
             "LDS scrub reached %d of %d CUs after %d rounds, below the floor %.3f",
             out->cus_seen, ctx->cus, rounds, o.min_cu_fraction);
    return -43;
  }
  out->ok = 1;
  snprintf(out->msg, sizeof(out->msg), "ok");
  return 0;
}

}  // namespace

extern "C" int cro_lds_scrub_run_records(int device, const struct CroLdsScrubOpts* opts,
                                         struct CroLdsScrubResult* out,
                                         struct CroLdsScrubRecord* records_out,
                                         int max_records) {
  memset(out, 0, sizeof(*out));
  out->first_dirty_word = out->first_bad_word = ~0u;
  out->xcd = out->se = out->sh = out->cu = -1;
  const double t0 = now_ms();
  out->rc = run_lds_scrub(device, opts, out, records_out, max_records);
  out->t_total_ms = now_ms() - t0;
  return out->rc;
}

extern "C" int cro_lds_scrub_run(int device, const struct CroLdsScrubOpts* opts,
                                 struct CroLdsScrubResult* out) {
  return cro_lds_scrub_run_records(device, opts, out, nullptr, 0);
}
