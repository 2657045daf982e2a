// cro_amd gfx950 data-movement probe stage: exact checks of the DPP crossbar,
// the LDS crossbar behind ds_swizzle / ds_permute / ds_bpermute, v_readlane /
// v_readfirstlane / v_writelane, the half-wave swaps, the transposed LDS reads
// and LDS-DMA on every CU and SIMD, with fault location.
//
// The other stages check arithmetic, LDS cells, atomics and visibility; a lane
// that receives its neighbour's register passes all of them.  This stage
// follows the shape of the formats stage: one 256-thread workgroup per CU (a
// CU's whole dynamic LDS is requested for placement, each wave uses 4 KiB of
// it), four waves, one per SIMD, and each wave runs every check and variant of
// cromovement.h `iters` times on payloads that change with the repeat.  A lane
// computes the word it must receive with plain integer arithmetic from the
// header's source maps, never through a cross-lane instruction, and compares
// bit for bit; mismatches are counted per wave and check with a 64-lane ballot
// and popcount, each wave reads where it ran (XCC_ID, HW_ID) and lane 0 writes
// one CroMovementRecord.  Workgroups are independent: no workgroup waits for
// another.  The host aggregates the records and launches the same grid again,
// a bounded number of times, while some CU or SIMD is still unseen.
//
// cro_movement_tile runs one wave of the same device functions on caller
// data, which is how the tests prove the maps at the head of cromovement.h.
//
// A library of its own (libcromovement.so): host plumbing from crohost.h.

#include <hip/hip_runtime.h>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "cromovement.h"
#include "crohost.h"

namespace {

constexpr int kWaves = kBlock / 64;
// ≈0.010 ms per repeat on an MI355X: 32 is the largest power of two that keeps
// the stage no more expensive than the formats stage's default (0.33 ms
// against 0.52 ms; 64 repeats cost 0.65 ms: profiles/movement_probe_mi355x.md)
constexpr int kDefaultIters = 32;
constexpr int kDefaultRounds = 4;
constexpr int kMaxRounds = 64;
constexpr int kMaxGrid = 1 << 16;
constexpr int kMaxIters = 1 << 16;
constexpr int kMaxTileGlobal = 8192;

#define LDS3 __attribute__((address_space(3)))
#define GLB1 __attribute__((address_space(1)))

typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x3 __attribute__((ext_vector_type(3)));

extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

// ---------------------------------------------------------------------------
// the instructions under test, one device function per check
// ---------------------------------------------------------------------------

template <int V>
__device__ inline uint32_t mov_dpp(uint32_t src, uint32_t old) {
  constexpr CroMovDpp d = cro_mov_dpp(V);
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, d.ctrl, d.row_mask, d.bank_mask,
                                               d.bound_ctrl != 0);
}

template <int V>
__device__ inline uint32_t mov_swizzle(uint32_t src) {
  return (uint32_t)__builtin_amdgcn_ds_swizzle((int)src, cro_mov_swizzle(V));
}

// idx is a lane number 0..63
template <int V>
__device__ inline uint32_t mov_bperm(uint32_t src, uint32_t idx) {
  if constexpr (V == 2)
    return (uint32_t)__builtin_amdgcn_ds_permute((int)(idx << 2), (int)src);
  else
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(idx << 2), (int)src);
}

template <int V>
__device__ inline void mov_plswap(uint32_t a, uint32_t b, uint32_t (&d)[CRO_MOV_MAX_REGS]) {
  if constexpr (V == 0) {
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    d[0] = r[0];
    d[1] = r[1];
  } else {
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    d[0] = r[0];
    d[1] = r[1];
  }
}

// `s` is wave-uniform: the lane select, the first active lane or the written lane
template <int V>
__device__ inline uint32_t mov_readlane(uint32_t src, uint32_t old, uint32_t lane, uint32_t s) {
  if constexpr (V == 0) {
    return (uint32_t)__builtin_amdgcn_readlane((int)src, (int)s);
  } else if constexpr (V == 1) {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)src);
  } else if constexpr (V == 2) {
    uint32_t r = old;
    if (lane >= s) r = (uint32_t)__builtin_amdgcn_readfirstlane((int)src);
    return r;
  } else {
    // no builtin: the value is a scalar a VALU instruction (v_readlane) wrote,
    // hence the wait inside the string; two scalar operands are one too many
    // for the constant bus, so the select goes through M0
    const uint32_t sel = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
    const uint32_t val = (uint32_t)__builtin_amdgcn_readlane((int)old, (int)sel);
    uint32_t keep;  // M0 is the compiler's: put it back
    asm volatile(
        "s_mov_b32 %1, m0\n\ts_mov_b32 m0, %3\n\ts_nop 4\n\tv_writelane_b32 %0, %2, m0\n\t"
        "s_mov_b32 m0, %1"
        : "+v"(src), "=&s"(keep)
        : "s"(val), "s"(sel));
    return src;
  }
}

// EXEC must be all ones and every lane's address in bounds and 8-byte aligned
template <int T>
__device__ inline void mov_tr(const unsigned char* p, uint32_t (&d)[CRO_MOV_MAX_REGS]) {
  if constexpr (T == CRO_MOV_TR16) {
    const i16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS3 i16x4*)p);
    const i32x2 w = __builtin_bit_cast(i32x2, r);
    d[0] = (uint32_t)w[0];
    d[1] = (uint32_t)w[1];
  } else if constexpr (T == CRO_MOV_TR8) {
    const i32x2 w = __builtin_amdgcn_ds_read_tr8_b64_v2i32((LDS3 i32x2*)p);
    d[0] = (uint32_t)w[0];
    d[1] = (uint32_t)w[1];
  } else if constexpr (T == CRO_MOV_TR4) {
    const i32x2 w = __builtin_amdgcn_ds_read_tr4_b64_v2i32((LDS3 i32x2*)p);
    d[0] = (uint32_t)w[0];
    d[1] = (uint32_t)w[1];
  } else {
    const i32x3 w = __builtin_amdgcn_ds_read_tr6_b96_v3i32((LDS3 i32x3*)p);
    d[0] = (uint32_t)w[0];
    d[1] = (uint32_t)w[1];
    d[2] = (uint32_t)w[2];
  }
}

// `g` is the lane's source address; `dst` the wave-uniform start of the
// destination, where lane 0's bytes must land
template <int V>
__device__ inline void mov_dma(const unsigned char* g, unsigned char* dst) {
  // (the builtin takes literals only)
  static_assert(cro_mov_dma_size(V) == (V == 1 ? 16 : 4) && cro_mov_dma_ioff(V) == (V == 2 ? 64 : 0),
                "the literals below follow cromovement.h");
  const GLB1 void* gp = (const GLB1 void*)g;
  if constexpr (V == 0) __builtin_amdgcn_global_load_lds(gp, (LDS3 void*)dst, 4, 0, 0);
  if constexpr (V == 1) __builtin_amdgcn_global_load_lds(gp, (LDS3 void*)dst, 16, 0, 0);
  if constexpr (V == 2) __builtin_amdgcn_global_load_lds(gp, (LDS3 void*)(dst - 64), 4, 64, 0);
}

// The DMA round trip of one wave: poison the region, transfer, read back with
// plain LDS reads.  d[0 .. n-1] are the data words 64 r + lane, d[n] the guard
// word of this lane.  Every thread of the workgroup calls it.
template <int V>
__device__ inline void dma_round(const unsigned char* g, unsigned char* my, uint32_t lane,
                                 uint32_t (&d)[CRO_MOV_MAX_REGS]) {
  constexpr int n = cro_mov_dma_size(V) / 4, total = 2 * CRO_MOV_GUARD + 64 * n;
  uint32_t* R = (uint32_t*)(my + CRO_MOV_DMA_BASE);
  for (uint32_t w = lane; w < (uint32_t)total; w += 64) R[w] = (uint32_t)CRO_MOV_POISON;
  __syncthreads();  // the poison is in LDS before the DMA writes over it
  mov_dma<V>(g, (unsigned char*)(R + CRO_MOV_GUARD));
  __syncthreads();  // waits for the wave's DMA (vmcnt) before the barrier
#pragma unroll
  for (int r = 0; r < n; ++r) d[r] = R[CRO_MOV_GUARD + 64 * r + lane];
  d[n] = lane < 32 ? R[lane] : R[CRO_MOV_GUARD + 64 * n + lane - 32];
  __syncthreads();  // read before the next variant poisons again
}

// calls f(std::integral_constant<int, v>) for the run-time variant v
template <int T, int V = 0, class F>
__device__ inline void with_variant(int v, F&& f) {
  if constexpr (V < cro_mov_variants(T)) {
    if (v == V)
      f(std::integral_constant<int, V>{});
    else
      with_variant<T, V + 1>(v, f);
  }
}

// calls f(std::integral_constant<int, v>) for every variant v of check T
template <int T, class F, int... V>
__device__ inline void each_variant_impl(F&& f, std::integer_sequence<int, V...>) {
  (f(std::integral_constant<int, V>{}), ...);
}
template <int T, class F>
__device__ inline void each_variant(F&& f) {
  each_variant_impl<T>(f, std::make_integer_sequence<int, cro_mov_variants(T)>{});
}

// ---------------------------------------------------------------------------
// raw tile entry: one wave, caller data, raw destination registers
// ---------------------------------------------------------------------------

struct TileArgs {
  const uint32_t* in;
  const int* addr;  // 64 per-lane values
  uint32_t* out;    // register-major: reg * 64 + lane
  int variant;
  int n_in_words;
};

template <int T>
__global__ __launch_bounds__(64) void tile_kernel(TileArgs t) {
  const uint32_t lane = threadIdx.x;  // exactly one wave of 64
  const uint32_t a = (uint32_t)t.addr[lane];
  const uint32_t a0 = (uint32_t)__builtin_amdgcn_readfirstlane(t.addr[0]);
  with_variant<T>(t.variant, [&](auto vc) {
    constexpr int V = decltype(vc)::value;
    uint32_t d[CRO_MOV_MAX_REGS] = {};
    if constexpr (T <= CRO_MOV_READLANE) {
      const uint32_t src = t.in[lane], old = t.in[64 + lane];
      if constexpr (T == CRO_MOV_DPP) d[0] = mov_dpp<V>(src, old);
      if constexpr (T == CRO_MOV_SWIZZLE) d[0] = mov_swizzle<V>(src);
      if constexpr (T == CRO_MOV_BPERMUTE) d[0] = mov_bperm<V>(src, a & 63u);
      if constexpr (T == CRO_MOV_PLSWAP) mov_plswap<V>(src, old, d);
      if constexpr (T == CRO_MOV_READLANE) d[0] = mov_readlane<V>(src, old, lane, a0 & 63u);
    } else if constexpr (T <= CRO_MOV_TR6) {
      for (uint32_t w = lane; w < (uint32_t)t.n_in_words; w += 64) ((uint32_t*)smem)[w] = t.in[w];
      __syncthreads();
      mov_tr<T>(smem + a, d);
    } else {
      dma_round<V>((const unsigned char*)t.in + a, smem, lane, d);
    }
#pragma unroll
    for (int r = 0; r < cro_mov_regs(T, V); ++r) t.out[r * 64 + lane] = d[r];
  });
}

// ---------------------------------------------------------------------------
// stage kernel
// ---------------------------------------------------------------------------

struct MovParams {
  const unsigned char* src;    // the fixed source buffer of the DMA check
  CroMovementRecord* records;  // this round's grid_blocks * 4 records
  uint32_t iters;
  uint32_t seed;
  uint32_t inj_want;  // self-test mode 1: the checks whose expected word is flipped
  uint32_t inj_mode;
  uint32_t inj_test;
  uint32_t inj_elem;
  uint32_t inj_key;
  uint32_t inj_flip;  // 1 << selftest_bit
};

// What one wave found in one check.  n_bad is wave-uniform (ballot counts);
// first and bits are per lane until reduce().
struct Tally {
  uint32_t n_bad = 0;
  uint32_t first = ~0u;
  uint32_t bits = 0;

  __device__ void add(uint32_t diff, uint32_t elem) {
    bits |= diff;
    const unsigned long long mask = __ballot(diff != 0);
    if (mask) {
      n_bad += (uint32_t)__popcll(mask);
      if (diff) first = elem < first ? elem : first;
    }
  }
  // every lane of the wave calls it (n_bad is uniform, so the branch is)
  __device__ void reduce() {
    if (!n_bad) return;
    for (int off = 32; off > 0; off >>= 1) {
      bits |= __shfl_xor(bits, off, 64);
      const uint32_t other = __shfl_xor(first, off, 64);
      first = other < first ? other : first;
    }
  }
};

// the self-test of this wave: data only
struct Inj {
  uint32_t want;  // checks whose expected word is flipped
  uint32_t got;   // check whose received word is flipped; ~0 = none
  uint32_t elem;  // ~0 = none
  uint32_t flip;
};

template <int T>
__device__ inline void cmp(Tally& t, const Inj& j, uint32_t got, uint32_t want, uint32_t elem) {
  if (elem == j.elem) {
    if ((j.want >> T) & 1u) want ^= j.flip;
    if (j.got == (uint32_t)T) got ^= j.flip;
  }
  t.add(got ^ want, elem);
}

__global__ __launch_bounds__(kBlock) void movement_kernel(MovParams p) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t xcc_id, hw_id;  // for the report only
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
  Inj inj;
  inj.want = p.inj_want;
  inj.got = p.inj_mode == 2 && cro_cov_cu_key(xcc_id, hw_id) == p.inj_key ? p.inj_test : ~0u;
  inj.elem = p.inj_mode ? p.inj_elem : ~0u;
  inj.flip = p.inj_flip;
  unsigned char* my = smem + wave * CRO_MOV_WAVE_LDS;

  Tally t[CRO_MOV_TESTS];
  for (uint32_t it = 0; it < p.iters; ++it) {
    // a zero the compiler cannot see through: every source word is rebuilt
    // and every instruction under test executed again in every repeat
    uint32_t z = 0;
    asm volatile("" : "+v"(z));
    const CroMovRt rt = cro_mov_rt(p.seed, it);
    const auto word = [&](int test, int v, int reg) {
      return cro_mov_payload(rt.salt, test, v, (int)lane, reg) + z;
    };

    each_variant<CRO_MOV_DPP>([&](auto vc) {
      constexpr int T = CRO_MOV_DPP, V = decltype(vc)::value;
      const uint32_t got = mov_dpp<V>(word(T, V, 0), word(T, V, 1));
      cmp<T>(t[T], inj, got, cro_mov_want(T, V, 0, (int)lane, &rt), cro_mov_elem(V, 0, lane));
    });
    each_variant<CRO_MOV_SWIZZLE>([&](auto vc) {
      constexpr int T = CRO_MOV_SWIZZLE, V = decltype(vc)::value;
      const uint32_t got = mov_swizzle<V>(word(T, V, 0));
      cmp<T>(t[T], inj, got, cro_mov_want(T, V, 0, (int)lane, &rt), cro_mov_elem(V, 0, lane));
    });
    each_variant<CRO_MOV_BPERMUTE>([&](auto vc) {
      constexpr int T = CRO_MOV_BPERMUTE, V = decltype(vc)::value;
      const uint32_t got = mov_bperm<V>(word(T, V, 0), cro_mov_bperm_idx(V, lane, &rt) + z);
      cmp<T>(t[T], inj, got, cro_mov_want(T, V, 0, (int)lane, &rt), cro_mov_elem(V, 0, lane));
    });
    each_variant<CRO_MOV_PLSWAP>([&](auto vc) {
      constexpr int T = CRO_MOV_PLSWAP, V = decltype(vc)::value;
      uint32_t d[CRO_MOV_MAX_REGS];
      mov_plswap<V>(word(T, V, 0), word(T, V, 1), d);
#pragma unroll
      for (int r = 0; r < 2; ++r)
        cmp<T>(t[T], inj, d[r], cro_mov_want(T, V, r, (int)lane, &rt), cro_mov_elem(V, r, lane));
    });
    each_variant<CRO_MOV_READLANE>([&](auto vc) {
      constexpr int T = CRO_MOV_READLANE, V = decltype(vc)::value;
      const uint32_t s = V == 0 ? rt.sel : V == 2 ? rt.fa : rt.wl;
      const uint32_t got = mov_readlane<V>(word(T, V, 0), word(T, V, 1), lane, s);
      cmp<T>(t[T], inj, got, cro_mov_want(T, V, 0, (int)lane, &rt), cro_mov_elem(V, 0, lane));
    });

    const auto transposed = [&](auto tc, auto vc) {
      constexpr int T = decltype(tc)::value, V = decltype(vc)::value;
      constexpr uint32_t words = cro_mov_tr_image_bytes(T, V) / 4;
      static_assert(words * 4 <= CRO_MOV_IMAGE_BYTES, "image larger than the wave's share");
      for (uint32_t w = lane; w < words; w += 64)
        ((uint32_t*)my)[w] = cro_mov_tr_image_word(T, V, (int)w, rt.salt) + z;
      __syncthreads();
      uint32_t d[CRO_MOV_MAX_REGS];
      mov_tr<T>(my + cro_mov_tr_addr(T, V, (int)lane), d);
#pragma unroll
      for (int r = 0; r < cro_mov_regs(T, V); ++r)
        cmp<T>(t[T], inj, d[r], cro_mov_tr_want(T, V, r, (int)lane, rt.salt),
               cro_mov_elem(V, r, lane));
      __syncthreads();  // read before the next image is written
    };
    each_variant<CRO_MOV_TR16>(
        [&](auto vc) { transposed(std::integral_constant<int, CRO_MOV_TR16>{}, vc); });
    each_variant<CRO_MOV_TR8>(
        [&](auto vc) { transposed(std::integral_constant<int, CRO_MOV_TR8>{}, vc); });
    each_variant<CRO_MOV_TR4>(
        [&](auto vc) { transposed(std::integral_constant<int, CRO_MOV_TR4>{}, vc); });
    each_variant<CRO_MOV_TR6>(
        [&](auto vc) { transposed(std::integral_constant<int, CRO_MOV_TR6>{}, vc); });

    each_variant<CRO_MOV_DMA>([&](auto vc) {
      constexpr int T = CRO_MOV_DMA, V = decltype(vc)::value;
      uint32_t d[CRO_MOV_MAX_REGS];
      dma_round<V>(p.src + cro_mov_dma_addr(V, (int)wave, (int)lane, &rt) + z, my, lane, d);
#pragma unroll
      for (int r = 0; r < cro_mov_regs(T, V); ++r)
        cmp<T>(t[T], inj, d[r], cro_mov_dma_want(V, r, (int)wave, (int)lane, &rt),
               cro_mov_elem(V, r, lane));
    });
  }

  uint32_t fail_mask = 0, n_bad = 0, first_bad = ~0u, bits_bad = 0;
#pragma unroll
  for (int k = CRO_MOV_TESTS - 1; k >= 0; --k) {
    t[k].reduce();
    if (t[k].n_bad) {  // the lowest failing check leads
      fail_mask |= 1u << k;
      n_bad = t[k].n_bad;
      first_bad = t[k].first;
      bits_bad = t[k].bits;
    }
  }
  if (lane == 0) {
    CroMovementRecord rec;
    rec.xcc_id = xcc_id;
    rec.hw_id = hw_id;
    rec.fail_mask = fail_mask;
    rec.n_bad = n_bad;
    rec.first_bad = first_bad;
    rec.bits_bad = bits_bad;
    rec.valid = 1;
    rec.reserved = 0;
    p.records[blockIdx.x * kWaves + wave] = rec;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// Per-device cached context (CtxBase, crohost.h): the DMA check's source
// buffer is uploaded once per device; the record buffer grows on demand.
struct MovCtx : CtxBase {
  int cus = 0;
  unsigned char* d_src = nullptr;
  RecordBuf<CroMovementRecord> records;
};
MovCtx g_mctx[kMaxDevices];

int prepare(MovCtx* ctx, int device, CroMovementResult* out) {
  if (ctx->ready) return 0;
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, device));
  ctx->cus = prop.multiProcessorCount;
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(movement_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, CRO_COV_MAX_LDS_BYTES));
  CHECK(hipEventCreate(&ctx->e0));
  CHECK(hipEventCreate(&ctx->e1));
  std::vector<uint32_t> src(CRO_MOV_SRC_WORDS);
  for (uint32_t i = 0; i < CRO_MOV_SRC_WORDS; ++i) src[i] = cro_mov_dma_word(i);
  CHECK(hipMalloc(&ctx->d_src, src.size() * 4));
  CHECK(hipMemcpy(ctx->d_src, src.data(), src.size() * 4, hipMemcpyHostToDevice));
  ctx->ready = 1;
  return 0;
}

int run_movement(int device, const CroMovementOpts* opts, CroMovementResult* out,
                 CroMovementRecord* records_out, int max_records) {
  CroMovementOpts o;
  memset(&o, 0, sizeof(o));
  if (opts) o = *opts;
  if (o.grid_blocks < 0 || o.grid_blocks > kMaxGrid) return bad_arg(out, "grid_blocks");
  if (o.iters < 0 || o.iters > kMaxIters) return bad_arg(out, "iters");
  if (o.max_rounds < 0 || o.max_rounds > kMaxRounds) return bad_arg(out, "max_rounds");
  // Unlike the compute and format stages, which stop at 1.0, this one allows
  // a floor above 1: no device can meet it, which is how the tests reach rc
  // -37 on clean data.
  if (!(o.min_cu_fraction >= 0.0 && o.min_cu_fraction <= 2.0))
    return bad_arg(out, "min_cu_fraction");
  const int iters = o.iters ? o.iters : kDefaultIters;
  const int max_rounds = o.max_rounds ? o.max_rounds : kDefaultRounds;
  // the self-test only ever names an element that exists
  if (o.selftest_mode < 0 || o.selftest_mode > 2) return bad_arg(out, "selftest_mode");
  uint32_t inj_want = 0;
  if (o.selftest_mode) {
    if (o.selftest_test < 0 || o.selftest_test >= CRO_MOV_TESTS)
      return bad_arg(out, "selftest_test");
    if (o.selftest_bit < 0 || o.selftest_bit > 31) return bad_arg(out, "selftest_bit");
    if (!cro_mov_elem_valid(o.selftest_test, o.selftest_elem))
      return bad_arg(out, "selftest_elem");
    if (o.selftest_mode == 1) inj_want = 1u << o.selftest_test;
    if (o.selftest_also) {
      const int t2 = o.selftest_also - 1;
      if (o.selftest_mode != 1 || t2 == o.selftest_test ||
          !cro_mov_elem_valid(t2, o.selftest_elem))
        return bad_arg(out, "selftest_also");
      inj_want |= 1u << t2;
    }
  } else if (o.selftest_also) {
    return bad_arg(out, "selftest_also");
  }

  std::unique_lock<std::mutex> lock;
  MovCtx* ctx = enter_device(g_mctx, device, lock, out->msg, sizeof(out->msg));
  if (ctx == nullptr) return -1;
  if (prepare(ctx, device, out) != 0) return -1;
  const int grid = o.grid_blocks ? o.grid_blocks : ctx->cus;
  if (grid < 1) return bad_arg(out, "device reports no compute units");
  const size_t per_round = (size_t)grid * kWaves;
  CHECK(ctx->records.reserve(per_round * (size_t)max_rounds));
  out->cus_expected = ctx->cus;
  out->grid_blocks = grid;
  out->iters = iters;

  MovParams p;
  memset(&p, 0, sizeof(p));
  p.src = ctx->d_src;
  p.iters = (uint32_t)iters;
  p.seed = o.seed;
  p.inj_want = inj_want;
  p.inj_mode = (uint32_t)o.selftest_mode;
  p.inj_test = (uint32_t)o.selftest_test;
  p.inj_elem = o.selftest_elem;
  p.inj_key = o.selftest_key;
  p.inj_flip = 1u << (o.selftest_bit & 31);

  const auto launch = [&](CroMovementRecord* d_round) {
    p.records = d_round;
    hipLaunchKernelGGL(movement_kernel, dim3(grid), dim3(kBlock), (size_t)CRO_COV_MAX_LDS_BYTES,
                       0, p);
  };
  if (run_rounds(*ctx, ctx->records.d, ctx->cus, per_round, max_rounds, launch,
                 cro_movement_aggregate, out, records_out, max_records) != 0)
    return -1;
  const CroMovementAgg& a = out->agg;
  if (a.waves_bad) {
    snprintf(out->failed_test, sizeof(out->failed_test), "%s",
             cro_mov_test_name(a.first_fail_mask));
    snprintf(out->msg, sizeof(out->msg),
             "data-movement mismatch in %s at xcd=%d se=%d sh=%d cu=%d simd=%d: variant %u "
             "register %u lane %u, bits 0x%08x; %llu of %llu waves bad on %d CUs",
             out->failed_test, a.xcd, a.se, a.sh, a.cu, a.simd, a.first_bad >> 12,
             (a.first_bad >> 6) & 63u, a.first_bad & 63u, a.bits_bad, a.waves_bad, a.waves_run,
             a.cus_bad);
    return -36;
  }
  return coverage_floor(out, ctx->cus, o.min_cu_fraction, -37);
}

template <int T>
void launch_tile(const TileArgs& t) {
  hipLaunchKernelGGL((tile_kernel<T>), dim3(1), dim3(64), (size_t)CRO_MOV_WAVE_LDS, 0, t);
}

}  // namespace

extern "C" int cro_movement_run_records(int device, const struct CroMovementOpts* opts,
                                        struct CroMovementResult* out,
                                        struct CroMovementRecord* records_out, int max_records) {
  clear_result(out, cro_movement_aggregate);
  const double t0 = now_ms();
  out->rc = run_movement(device, opts, out, records_out, max_records);
  out->t_total_ms = now_ms() - t0;
  return out->rc;
}

extern "C" int cro_movement_run(int device, const struct CroMovementOpts* opts,
                                struct CroMovementResult* out) {
  return cro_movement_run_records(device, opts, out, nullptr, 0);
}

extern "C" int cro_movement_tile(int device, int test, int variant, const void* in,
                                 int n_in_bytes, const int* addr, void* out, int n_out_bytes) {
  if (test < 0 || test >= CRO_MOV_TESTS || variant < 0 || variant >= cro_mov_variants(test))
    return -10;
  if (in == nullptr || out == nullptr) return -10;
  const int out_bytes = cro_mov_regs(test, variant) * 256;
  if (n_out_bytes != out_bytes || n_in_bytes <= 0 || n_in_bytes % 4 != 0) return -10;
  int h_addr[64] = {};
  if (addr) memcpy(h_addr, addr, sizeof(h_addr));
  // every address is checked here: the kernel trusts it
  if (test <= CRO_MOV_READLANE) {
    if (n_in_bytes != 2 * 64 * 4) return -10;
    const bool needs = test == CRO_MOV_BPERMUTE || (test == CRO_MOV_READLANE && variant != 1);
    if (needs && addr == nullptr) return -10;
    for (int l = 0; l < 64; ++l)
      if (h_addr[l] < 0 || h_addr[l] > 63) return -10;
    if (test == CRO_MOV_READLANE && variant == 2 && h_addr[0] == 0) return -10;
  } else if (test <= CRO_MOV_TR6) {
    if (addr == nullptr || n_in_bytes > CRO_MOV_IMAGE_BYTES) return -10;
    const int nbytes = cro_mov_tr(test).nbytes;
    for (int l = 0; l < 64; ++l)
      if (h_addr[l] < 0 || h_addr[l] % 8 != 0 || h_addr[l] + nbytes > n_in_bytes) return -10;
  } else {
    if (addr == nullptr || n_in_bytes > kMaxTileGlobal) return -10;
    const int size = cro_mov_dma_size(variant), ioff = cro_mov_dma_ioff(variant);
    for (int l = 0; l < 64; ++l)
      if (h_addr[l] < 0 || h_addr[l] % size != 0 || h_addr[l] + ioff + size > n_in_bytes)
        return -10;
  }
  if (hipSetDevice(device) != hipSuccess) return -1;
  DevBuf<uint32_t> d_in, d_out;
  DevBuf<int> d_addr;
  const auto run = [&]() -> hipError_t {
    TRY(d_in.alloc((size_t)n_in_bytes));
    TRY(d_out.alloc((size_t)out_bytes));
    TRY(d_addr.alloc(sizeof(h_addr)));
    TRY(hipMemcpy(d_in.get(), in, (size_t)n_in_bytes, hipMemcpyHostToDevice));
    TRY(hipMemcpy(d_addr.get(), h_addr, sizeof(h_addr), hipMemcpyHostToDevice));
    TRY(hipMemset(d_out.get(), 0, (size_t)out_bytes));
    const TileArgs t = {d_in.get(), d_addr.get(), d_out.get(), variant, n_in_bytes / 4};
    switch (test) {
      case CRO_MOV_DPP: launch_tile<CRO_MOV_DPP>(t); break;
      case CRO_MOV_SWIZZLE: launch_tile<CRO_MOV_SWIZZLE>(t); break;
      case CRO_MOV_BPERMUTE: launch_tile<CRO_MOV_BPERMUTE>(t); break;
      case CRO_MOV_PLSWAP: launch_tile<CRO_MOV_PLSWAP>(t); break;
      case CRO_MOV_READLANE: launch_tile<CRO_MOV_READLANE>(t); break;
      case CRO_MOV_TR16: launch_tile<CRO_MOV_TR16>(t); break;
      case CRO_MOV_TR8: launch_tile<CRO_MOV_TR8>(t); break;
      case CRO_MOV_TR4: launch_tile<CRO_MOV_TR4>(t); break;
      case CRO_MOV_TR6: launch_tile<CRO_MOV_TR6>(t); break;
      default: launch_tile<CRO_MOV_DMA>(t); break;
    }
    TRY(hipGetLastError());
    return hipMemcpy(out, d_out.get(), (size_t)out_bytes, hipMemcpyDeviceToHost);
  };
  return run() == hipSuccess ? 0 : -1;
}
