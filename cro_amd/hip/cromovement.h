// Data-movement probe stage: exact checks of the hardware that moves data
// between lanes and into LDS without arithmetic, with fault location.
//
// Everything the host decides lives here: for every check and variant the
// source map (which lane, register and bit field every destination lane,
// register and bit field must receive), the payload hash, the LDS and global
// images, the per-wave record, the aggregation and the C ABI of
// libcromovement.so.  One definition shared by the device kernel
// (movement.hip), the native agent, a host-only test program and the numpy
// mirrors of nodeops/movement.py.  Plain C++: a host compiler without HIP can
// include it.
//
// Checks, in fail-mask bit order (cro_mov_test_name), and their variants:
//
//   0 dpp            v_mov_b32_dpp (the compiler may fold the control into
//                    another VALU instruction: still the DPP path)
//        0 quad_perm:[1,3,0,2]          7 wave_shr:1 bound_ctrl (lane 0 reads 0)
//        1 row_shl:1 bound_ctrl         8 wave_rol:1
//          (lane 15 of a row reads 0)   9 wave_ror:1
//        2 row_shr:3 (lanes 0..2 of    10 row_bcast:15 row_mask:0xa
//          a row keep `old`)           11 row_bcast:31 row_mask:0xc
//        3 row_ror:5                   12 row_shr:1 bank_mask:0x5 (banks 1 and
//        4 row_mirror                     3 and lane 0 of a row keep `old`)
//        5 row_half_mirror
//        6 wave_shl:1 (lane 63 keeps `old`)
//   1 swizzle        ds_swizzle_b32
//        0 quad-perm mode [2,0,3,1]     3 broadcast: and 0x18 or 0x05
//        1 swap: xor 0x01               4 mixed: and 0x17 or 0x08 xor 0x12
//        2 reverse: xor 0x1f              (bit-mask mode works per 32 lanes)
//   2 bpermute       ds_bpermute_b32 (0, 1), ds_permute_b32 (2); run-time
//                    indices (i * a + b) & 63, a odd, from the seed
//        0 pull through the permutation
//        1 pull through the many-to-one map ((i >> 1) * a + b) & 63
//        2 push through the permutation
//   3 permlane_swap  0 v_permlane16_swap_b32, 1 v_permlane32_swap_b32;
//                    destination register 0 is the first result, 1 the second
//   4 readlane       0 v_readlane_b32, select (sel0(seed) + repeat) & 63
//                    1 v_readfirstlane_b32 under full EXEC
//                    2 v_readfirstlane_b32 with lanes fa..63 active; the
//                      others keep `old`
//                    3 v_writelane_b32 of lane wl's `old` word into lane wl
//   5 lds_tr16       ds_read_b64_tr_b16: row stride 0 plain (32 B), 1 padded (40 B)
//   6 lds_tr8        ds_read_b64_tr_b8:  row stride 0 plain (16 B), 1 padded (24 B)
//   7 lds_tr4        ds_read_b64_tr_b4:  0 every nibble carries its source row
//                    (stride 8 B), 1 its source column (stride 16 B)
//   8 lds_tr6        ds_read_b96_tr_b6:  0 source row (stride 16 B), 1 source
//                    column (stride 32 B), in 6-bit fields
//   9 lds_dma        0 global_load_lds_dword, 1 global_load_lds_dwordx4,
//                    2 global_load_lds_dword offset:64; per-lane source
//                    addresses from a seeded permutation of the wave's chunks
//
// An element of a check is (variant << 12) | (register << 6) | lane: that is
// what first_bad and selftest_elem hold.
//
// Maps (proved on an MI355X with cro_movement_tile; the sweeps are recorded in
// profiles/movement_probe_mi355x.md).  `src` is source register 0, `old`
// source register 1; r = lane >> 4 is the row, i = lane & 15.
//
//   dpp       a lane whose row is not in row_mask or whose bank ((i >> 2)) is
//             not in bank_mask keeps `old`; an invalid source reads 0 with
//             bound_ctrl and keeps `old` without.  quad_perm: lane 4k+j reads
//             4k+perm[j].  row_shl:n reads i+n, row_shr:n reads i-n (invalid
//             outside the row), row_ror:n reads (i-n) & 15, row_mirror reads
//             15-i, row_half_mirror reads i ^ 7, wave_shl:1 reads lane+1,
//             wave_shr:1 lane-1 (invalid outside the wave), wave_rol:1 and
//             wave_ror:1 the same modulo 64, row_bcast:15 reads lane 16r-1
//             (row 0 invalid), row_bcast:31 reads lane 31 (rows 0, 1 invalid).
//   swizzle   quad-perm mode as dpp quad_perm; bit-mask mode: lane l reads
//             (l & 32) | ((((l & 31) & and) | or) ^ xor).
//   bpermute  pull: lane i reads lane idx[i]; push: lane idx[i] receives lane i.
//   permlane16_swap(a, b): result 0 is a with its odd rows replaced by b's
//             even rows one below; result 1 is b with its even rows replaced
//             by a's odd rows one above.  permlane32_swap: result 0 is
//             {a.lo, b.lo}, result 1 {a.hi, b.hi} (lo = lanes 0..31).
//   transposed reads, per group of 16 consecutive lanes: the group's block is
//             F rows x 16 columns of b-bit elements, F = 64 / b (b = 16, 8,
//             4) or 96 / 6 = 16: 4x16, 8x16, 16x16, 16x16.  A row is 16 * b
//             bits; the instruction's 8 (12) bytes are one P-th of it, P = 4,
//             2, 1, 1.  Lane P*q+p of the group supplies the address of row
//             q, columns (16/P)*p .. ; lane i receives column i, row q in its
//             b-bit field q (field q is at bit q*b of the lane's 64 or 96
//             bits, little endian across the destination registers).
//   lds_dma   LDS destination: the wave-uniform base + instruction offset +
//             lane * size; global source: the lane's address + the same
//             instruction offset.
//
// Instructions (hipcc --offload-arch=gfx950 -O3, read in the stage's
// assembly): v_mov_b32_dpp with quad_perm, row_shl, row_shr, row_ror,
// row_mirror, row_half_mirror, wave_shl, wave_shr, wave_rol, wave_ror,
// row_bcast:15, row_bcast:31, bound_ctrl, row_mask and bank_mask controls;
// ds_swizzle_b32; ds_bpermute_b32; ds_permute_b32; v_permlane16_swap_b32;
// v_permlane32_swap_b32; v_readlane_b32; v_readfirstlane_b32;
// v_writelane_b32; ds_read_b64_tr_b16 / _tr_b8 / _tr_b4; ds_read_b96_tr_b6;
// global_load_lds_dword; global_load_lds_dwordx4.  No scratch.
//
// Not covered: the v_cvt_scalef32_* conversions, SDWA, buffer_load .. lds,
// the DMA's cache-policy bits and its 1-, 2- and 12-byte sizes, ds_bpermute
// indices outside 0..63, transposed reads under partial EXEC, rates and bank
// conflicts.
#pragma once

#include "crocoverage.h"

enum {
  CRO_MOV_DPP = 0,
  CRO_MOV_SWIZZLE = 1,
  CRO_MOV_BPERMUTE = 2,
  CRO_MOV_PLSWAP = 3,
  CRO_MOV_READLANE = 4,
  CRO_MOV_TR16 = 5,
  CRO_MOV_TR8 = 6,
  CRO_MOV_TR4 = 7,
  CRO_MOV_TR6 = 8,
  CRO_MOV_DMA = 9,
  CRO_MOV_TESTS = 10,
};

enum {
  CRO_MOV_SRC_ZERO = -1,       // source code: the destination reads 0
  CRO_MOV_WAVE_LDS = 4096,     // bytes of LDS a wave uses
  CRO_MOV_IMAGE_BYTES = 2048,  // of which its transposed-read image may take
  CRO_MOV_DMA_BASE = 2048,     // and where its DMA region starts
  CRO_MOV_GUARD = 32,          // poisoned words either side of the DMA destination
  CRO_MOV_DMA_OFFSET = 64,     // the instruction offset of lds_dma variant 2
  CRO_MOV_SRC_WORDS = 2048,    // words of the device source buffer
  CRO_MOV_MAX_REGS = 5,        // destination registers of a check, at most
  CRO_MOV_POISON = 0x5EEDF00D,
};

static const char* const kCroMovTestNames[CRO_MOV_TESTS] = {
    "dpp",      "swizzle", "bpermute", "permlane_swap", "readlane",
    "lds_tr16", "lds_tr8", "lds_tr4",  "lds_tr6",       "lds_dma"};

static inline const char* cro_mov_test_name(uint32_t fail_mask) {
  for (int t = 0; t < CRO_MOV_TESTS; ++t)
    if (fail_mask & (1u << t)) return kCroMovTestNames[t];
  return "";
}

CRO_COV_HD static inline constexpr int cro_mov_variants(int test) {
  return test == CRO_MOV_DPP        ? 13
         : test == CRO_MOV_SWIZZLE  ? 5
         : test == CRO_MOV_BPERMUTE ? 3
         : test == CRO_MOV_PLSWAP   ? 2
         : test == CRO_MOV_READLANE ? 4
         : test == CRO_MOV_DMA      ? 3
                                    : 2;
}

// destination registers of a variant (lds_dma: the data and one of guard words)
CRO_COV_HD static inline constexpr int cro_mov_regs(int test, int variant) {
  return test == CRO_MOV_PLSWAP || test == CRO_MOV_TR16 || test == CRO_MOV_TR8 ||
                 test == CRO_MOV_TR4
             ? 2
         : test == CRO_MOV_TR6 ? 3
         : test == CRO_MOV_DMA ? (variant == 1 ? 5 : 2)
                               : 1;
}

CRO_COV_HD static inline constexpr uint32_t cro_mov_elem(int variant, int reg, int lane) {
  return ((uint32_t)variant << 12) | ((uint32_t)reg << 6) | (uint32_t)lane;
}

CRO_COV_HD static inline bool cro_mov_elem_valid(int test, uint32_t elem) {
  const int v = (int)(elem >> 12), r = (int)((elem >> 6) & 63u);
  return test >= 0 && test < CRO_MOV_TESTS && v < cro_mov_variants(test) &&
         r < cro_mov_regs(test, v);
}

// -- payloads and run-time values -----------------------------------------------------

CRO_COV_HD static inline uint32_t cro_mov_lcg(uint32_t s) { return s * 1664525u + 1013904223u; }

CRO_COV_HD static inline uint32_t cro_mov_salt(uint32_t seed, uint32_t rep) {
  return cro_mov_lcg(cro_mov_lcg(seed ^ ((rep + 1u) * 0x9e3779b9u)));
}

// the word source register `reg` of lane `lane` holds: distinct for distinct
// (check, variant, lane, register), the hash being a bijection
CRO_COV_HD static inline uint32_t cro_mov_payload(uint32_t salt, int test, int variant, int lane,
                                                  int reg) {
  const uint32_t key = ((uint32_t)test << 20) | cro_mov_elem(variant, reg, lane);
  return cro_mov_lcg(cro_mov_lcg(salt ^ key));
}

// what repeat `rep` of a run with `seed` uses beside its salt
struct CroMovRt {
  uint32_t salt;
  uint32_t sel;  // v_readlane's lane select: sweeps all lanes over 64 repeats
  uint32_t fa;   // first active lane of the partial-EXEC v_readfirstlane
  uint32_t wl;   // the lane v_writelane writes
  uint32_t a;    // permutation (i * a + b) & 63, a odd
  uint32_t b;
};

CRO_COV_HD static inline CroMovRt cro_mov_rt(uint32_t seed, uint32_t rep) {
  CroMovRt rt;
  rt.salt = cro_mov_salt(seed, rep);
  const uint32_t h = cro_mov_lcg(rt.salt ^ 0x5bd1e995u) >> 8;
  rt.sel = ((cro_mov_lcg(seed) >> 26) + rep) & 63u;
  rt.fa = 1u + h % 63u;  // 1..63: never the full mask
  rt.wl = (h >> 6) & 63u;
  rt.a = ((h >> 12) & 63u) | 1u;
  if (rt.a == 1u || rt.a == 63u) rt.a = 37u;  // neither the identity nor its mirror image
  rt.b = (h >> 18) & 63u;
  return rt;
}

// the inverse of odd a modulo 64
CRO_COV_HD static inline uint32_t cro_mov_inv64(uint32_t a) {
  uint32_t x = a;  // correct to 3 bits
  x *= 2u - a * x;
  x *= 2u - a * x;
  return x & 63u;
}

// -- checks 0..4: source codes ----------------------------------------------------------
// A source code is (register << 6) | lane of the source word (register 0 src,
// 1 old), or CRO_MOV_SRC_ZERO.

struct CroMovDpp {
  int ctrl, row_mask, bank_mask, bound_ctrl;
};

CRO_COV_HD static inline constexpr CroMovDpp cro_mov_dpp(int v) {
  return v == 0    ? CroMovDpp{0x8D, 0xf, 0xf, 0}   // quad_perm:[1,3,0,2]
         : v == 1  ? CroMovDpp{0x101, 0xf, 0xf, 1}  // row_shl:1
         : v == 2  ? CroMovDpp{0x113, 0xf, 0xf, 0}  // row_shr:3
         : v == 3  ? CroMovDpp{0x125, 0xf, 0xf, 0}  // row_ror:5
         : v == 4  ? CroMovDpp{0x140, 0xf, 0xf, 0}  // row_mirror
         : v == 5  ? CroMovDpp{0x141, 0xf, 0xf, 0}  // row_half_mirror
         : v == 6  ? CroMovDpp{0x130, 0xf, 0xf, 0}  // wave_shl:1
         : v == 7  ? CroMovDpp{0x138, 0xf, 0xf, 1}  // wave_shr:1
         : v == 8  ? CroMovDpp{0x134, 0xf, 0xf, 0}  // wave_rol:1
         : v == 9  ? CroMovDpp{0x13C, 0xf, 0xf, 0}  // wave_ror:1
         : v == 10 ? CroMovDpp{0x142, 0xa, 0xf, 0}  // row_bcast:15
         : v == 11 ? CroMovDpp{0x143, 0xc, 0xf, 0}  // row_bcast:31
                   : CroMovDpp{0x111, 0xf, 0x5, 0};  // row_shr:1
}

CRO_COV_HD static inline int cro_mov_dpp_src(int v, int lane) {
  const CroMovDpp d = cro_mov_dpp(v);
  const int row = lane >> 4, i = lane & 15, keep = 64 | lane;
  if (!((d.row_mask >> row) & 1) || !((d.bank_mask >> (i >> 2)) & 1)) return keep;
  const int c = d.ctrl, n = c & 15;
  int s = 0;
  bool valid = true;
  if (c < 0x100) {
    s = (lane & ~3) | ((c >> (2 * (lane & 3))) & 3);
  } else if (c < 0x110) {  // row_shl
    valid = i + n < 16;
    s = lane + n;
  } else if (c < 0x120) {  // row_shr
    valid = i - n >= 0;
    s = lane - n;
  } else if (c < 0x130) {  // row_ror
    s = (lane & ~15) | ((i - n) & 15);
  } else if (c == 0x130) {
    valid = lane < 63;
    s = lane + 1;
  } else if (c == 0x134) {
    s = (lane + 1) & 63;
  } else if (c == 0x138) {
    valid = lane > 0;
    s = lane - 1;
  } else if (c == 0x13C) {
    s = (lane - 1) & 63;
  } else if (c == 0x140) {
    s = (lane & ~15) | (15 - i);
  } else if (c == 0x141) {
    s = lane ^ 7;
  } else if (c == 0x142) {
    valid = row > 0;
    s = 16 * row - 1;
  } else {
    valid = row > 1;
    s = 31;
  }
  if (!valid) return d.bound_ctrl ? (int)CRO_MOV_SRC_ZERO : keep;
  return s;
}

// ds_swizzle offsets: bit 15 quad-perm mode; else and | or << 5 | xor << 10
CRO_COV_HD static inline constexpr int cro_mov_swizzle(int v) {
  return v == 0   ? 0x8072
         : v == 1 ? 0x041F
         : v == 2 ? 0x7C1F
         : v == 3 ? 0x00B8
                  : 0x4917;
}

CRO_COV_HD static inline int cro_mov_swizzle_src(int v, int lane) {
  const int o = cro_mov_swizzle(v);
  if (o & 0x8000) return (lane & ~3) | ((o >> (2 * (lane & 3))) & 3);
  return (lane & 32) | ((((lane & 31) & (o & 31)) | ((o >> 5) & 31)) ^ ((o >> 10) & 31));
}

// the index lane `lane` passes to ds_bpermute / ds_permute (a lane number; the
// instruction takes it times 4)
CRO_COV_HD static inline uint32_t cro_mov_bperm_idx(int v, uint32_t lane, const CroMovRt* rt) {
  return ((v == 1 ? lane >> 1 : lane) * rt->a + rt->b) & 63u;
}

CRO_COV_HD static inline int cro_mov_bperm_src(int v, int lane, const CroMovRt* rt) {
  if (v != 2) return (int)cro_mov_bperm_idx(v, (uint32_t)lane, rt);
  return (int)((((uint32_t)lane - rt->b) * cro_mov_inv64(rt->a)) & 63u);
}

CRO_COV_HD static inline int cro_mov_plswap_src(int v, int reg, int lane) {
  if (v == 0) {
    const int odd = (lane >> 4) & 1;
    if (reg == 0) return odd ? (64 | (lane - 16)) : lane;
    return odd ? (64 | lane) : lane + 16;
  }
  if (reg == 0) return lane < 32 ? lane : (64 | (lane - 32));
  return lane < 32 ? lane + 32 : (64 | lane);
}

CRO_COV_HD static inline int cro_mov_readlane_src(int v, int lane, const CroMovRt* rt) {
  if (v == 0) return (int)rt->sel;
  if (v == 1) return 0;
  if (v == 2) return lane >= (int)rt->fa ? (int)rt->fa : (64 | lane);
  return lane == (int)rt->wl ? (64 | lane) : lane;
}

// source code of destination (variant, register, lane) of checks 0..4
CRO_COV_HD static inline int cro_mov_src(int test, int v, int reg, int lane, const CroMovRt* rt) {
  switch (test) {
    case CRO_MOV_DPP: return cro_mov_dpp_src(v, lane);
    case CRO_MOV_SWIZZLE: return cro_mov_swizzle_src(v, lane);
    case CRO_MOV_BPERMUTE: return cro_mov_bperm_src(v, lane, rt);
    case CRO_MOV_PLSWAP: return cro_mov_plswap_src(v, reg, lane);
    default: return cro_mov_readlane_src(v, lane, rt);
  }
}

CRO_COV_HD static inline uint32_t cro_mov_want(int test, int v, int reg, int lane,
                                               const CroMovRt* rt) {
  const int s = cro_mov_src(test, v, reg, lane, rt);
  return s < 0 ? 0u : cro_mov_payload(rt->salt, test, v, s & 63, s >> 6);
}

// -- checks 5..8: transposed LDS reads --------------------------------------------------

struct CroMovTr {
  int bits;    // of an element
  int rows;    // of a 16-lane group's block: the fields a lane receives
  int per;     // lanes that supply one row
  int nbytes;  // a lane reads
};

CRO_COV_HD static inline constexpr CroMovTr cro_mov_tr(int test) {
  return test == CRO_MOV_TR16  ? CroMovTr{16, 4, 4, 8}
         : test == CRO_MOV_TR8 ? CroMovTr{8, 8, 2, 8}
         : test == CRO_MOV_TR4 ? CroMovTr{4, 16, 1, 8}
                               : CroMovTr{6, 16, 1, 12};
}

// row stride in bytes: a multiple of 8
CRO_COV_HD static inline constexpr int cro_mov_tr_stride(int test, int v) {
  return test == CRO_MOV_TR16  ? (v ? 40 : 32)
         : test == CRO_MOV_TR8 ? (v ? 24 : 16)
         : test == CRO_MOV_TR4 ? (v ? 16 : 8)
                               : (v ? 32 : 16);
}

CRO_COV_HD static inline constexpr int cro_mov_tr_image_bytes(int test, int v) {
  return 4 * cro_mov_tr(test).rows * cro_mov_tr_stride(test, v);
}

// byte offset, in the wave's image, lane `lane` passes to the instruction
CRO_COV_HD static inline int cro_mov_tr_addr(int test, int v, int lane) {
  const CroMovTr t = cro_mov_tr(test);
  const int stride = cro_mov_tr_stride(test, v), g = lane >> 4, j = lane & 15;
  return g * t.rows * stride + (j / t.per) * stride + (j % t.per) * t.nbytes;
}

// the element (block, row, col) of the image
CRO_COV_HD static inline uint32_t cro_mov_tr_code(int test, int v, int block, int row, int col,
                                                  uint32_t salt) {
  switch (test) {
    case CRO_MOV_TR16:
      return ((uint32_t)(block * 64 + row * 16 + col) * 0x9E35u + salt) & 0xFFFFu;
    case CRO_MOV_TR8:
      return ((uint32_t)(row * 16 + col) * 0x9Du + (uint32_t)block * 0x35u + salt) & 0xFFu;
    case CRO_MOV_TR4:
      return ((uint32_t)(v ? col : row) ^ salt ^ (uint32_t)(block * 5)) & 0xFu;
    default:
      return ((uint32_t)((v ? col : row) | (block << 4)) ^ salt) & 0x3Fu;
  }
}

// 32-bit word `w` of a little-endian string of `n` fields of `bits` bits,
// field k being f(k)
#define CRO_MOV_PACK(word, w, n, bits, expr)                                      \
  do {                                                                            \
    word = 0u;                                                                    \
    for (int k = 0; k < (n); ++k) {                                               \
      const int lo_ = k * (bits)-32 * (w);                                        \
      if (lo_ <= -(bits) || lo_ >= 32) continue;                                  \
      const uint32_t f_ = (expr);                                                 \
      word |= lo_ >= 0 ? f_ << lo_ : f_ >> -lo_;                                  \
    }                                                                             \
  } while (0)

// 32-bit word `w` of the wave's image (pad words are poison)
CRO_COV_HD static inline uint32_t cro_mov_tr_image_word(int test, int v, int w, uint32_t salt) {
  const CroMovTr t = cro_mov_tr(test);
  const int stride = cro_mov_tr_stride(test, v);
  const int off = 4 * w, block = off / (t.rows * stride), row = off / stride % t.rows;
  const int in_row = off % stride / 4;
  if (in_row * 32 >= 16 * t.bits) return (uint32_t)CRO_MOV_POISON ^ (uint32_t)w;
  uint32_t word;
  CRO_MOV_PACK(word, in_row, 16, t.bits, cro_mov_tr_code(test, v, block, row, k, salt));
  return word;
}

// destination register `reg` of lane `lane`: column lane & 15 of the group's
// block, row q in field q
CRO_COV_HD static inline uint32_t cro_mov_tr_want(int test, int v, int reg, int lane,
                                                  uint32_t salt) {
  const CroMovTr t = cro_mov_tr(test);
  uint32_t word;
  CRO_MOV_PACK(word, reg, t.rows, t.bits,
               cro_mov_tr_code(test, v, lane >> 4, k, lane & 15, salt));
  return word;
}

// -- check 9: LDS-DMA -------------------------------------------------------------------

CRO_COV_HD static inline constexpr int cro_mov_dma_size(int v) { return v == 1 ? 16 : 4; }
CRO_COV_HD static inline constexpr int cro_mov_dma_ioff(int v) {
  return v == 2 ? (int)CRO_MOV_DMA_OFFSET : 0;
}

// the fixed content of the device source buffer
CRO_COV_HD static inline uint32_t cro_mov_dma_word(uint32_t i) {
  return cro_mov_lcg(cro_mov_lcg(i ^ 0x6d6f7631u));
}

// byte address, in the source buffer, lane `lane` of wave `wave` passes: a
// permutation of the wave's 64 chunks
CRO_COV_HD static inline uint32_t cro_mov_dma_addr(int v, int wave, int lane, const CroMovRt* rt) {
  const uint32_t chunk = (((uint32_t)lane * rt->a + rt->b + (uint32_t)v) & 63u);
  return (uint32_t)wave * 1024u + chunk * (uint32_t)cro_mov_dma_size(v);
}

// What read-back register `reg` of lane `lane` must hold.  The read-back is
// lane-linear: registers 0 .. n-1 are words 64 reg + lane of the destination,
// register n is the guard (lanes 0..31 the words before it, 32..63 after).
CRO_COV_HD static inline uint32_t cro_mov_dma_want(int v, int reg, int wave, int lane,
                                                   const CroMovRt* rt) {
  const int n = cro_mov_dma_size(v) / 4;
  if (reg >= n) return (uint32_t)CRO_MOV_POISON;
  const int w = 64 * reg + lane;
  const uint32_t addr = cro_mov_dma_addr(v, wave, w / n, rt) + (uint32_t)cro_mov_dma_ioff(v);
  return cro_mov_dma_word(addr / 4u + (uint32_t)(w % n));
}

// -- record and aggregation -------------------------------------------------------------

// One per wave and round, written by lane 0.  n_bad, first_bad and bits_bad
// belong to the failing check with the lowest mask bit (the one
// cro_mov_test_name names): the compared words that differed over all
// repeats, the lowest bad element and the OR of got ^ want.
struct CroMovementRecord {
  uint32_t xcc_id;     // raw XCC_ID register
  uint32_t hw_id;      // raw HW_ID register
  uint32_t fail_mask;  // bit t: check t
  uint32_t n_bad;
  uint32_t first_bad;  // ~0 = none
  uint32_t bits_bad;
  uint32_t valid;  // 1 once a wave wrote the record
  uint32_t reserved;
};

struct CroMovementAgg {
  unsigned long long waves_run;           // valid records
  unsigned long long waves_bad;           // records with a non-zero fail mask
  unsigned long long bad[CRO_MOV_TESTS];  // bad_<check>: bad waves per check
  int cus_seen;                           // distinct CU keys
  int xcds_seen;
  int simds_seen;  // distinct (CU key, SIMD) pairs
  int cus_bad;     // distinct CU keys with a bad wave
  // the first bad wave (lowest record index); -1 / 0 when there is none
  int xcd, se, sh, cu, simd;
  unsigned int fail_mask;  // every check that failed anywhere
  unsigned int first_fail_mask;
  unsigned int n_bad;
  unsigned int first_bad;
  unsigned int bits_bad;
  long long first_bad_index;  // index of the first bad record; -1 = none
};

// cro_wave_summarize (crocoverage.h); over no records the cleared aggregate.
static inline void cro_movement_aggregate(const CroMovementRecord* records, size_t n,
                                          CroMovementAgg* out) {
  CroWaveSummary s;
  cro_wave_summarize(records, n, &s);
  cro_wave_common(s, out);
  for (int t = 0; t < CRO_MOV_TESTS; ++t) out->bad[t] = s.bad[t];
  out->fail_mask = s.fail_mask;
}

// -- C ABI (libcromovement.so) ----------------------------------------------------------

// Zero takes the library default.  The selftest_* options are for tests: they
// alter data only, in bounds.
//   mode 1  bit selftest_bit of the EXPECTED word of element selftest_elem of
//           check selftest_test is flipped in every wave (with selftest_also
//           = 1 + t2 the same bit of the same element of check t2 as well)
//   mode 2  that bit of the RECEIVED word is flipped on the waves whose CU key
//           (cro_cov_cu_key) is selftest_key
struct CroMovementOpts {
  int grid_blocks;  // workgroups; default one per CU
  int iters;        // repeats of all checks per wave
  int max_rounds;   // bounded relaunch while a CU or SIMD is unseen
  unsigned int seed;
  int selftest_mode;
  int selftest_test;
  int selftest_bit;  // 0..31
  unsigned int selftest_elem;
  unsigned int selftest_key;
  int selftest_also;
  double min_cu_fraction;  // > 0: fewer CUs seen than this fraction is rc -37
};

struct CroMovementResult {
  int ok;
  int rc;  // 0 ok, -1 HIP error or bad argument, -36 mismatch, -37 CU-coverage floor
  int cus_expected;
  int rounds;
  struct CroMovementAgg agg;
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

int cro_movement_run(int device, const struct CroMovementOpts* opts,
                     struct CroMovementResult* out);

// cro_movement_run, and the rounds' raw records (at most max_records), round-major.
int cro_movement_run_records(int device, const struct CroMovementOpts* opts,
                             struct CroMovementResult* out,
                             struct CroMovementRecord* records_out, int max_records);

// One wave of the stage's own device function for `test` and `variant` on
// caller data (for tests; this is what proves the maps).  `out` receives the
// raw destination registers, register-major: word reg * 64 + lane,
// cro_mov_regs(test, variant) * 256 bytes.
//   checks 0..4  `in` is 2 x 64 words (src, then old); `addr` holds lane
//                numbers 0..63: per lane the bpermute index, in addr[0] the
//                readlane select, first active lane (1..63) or written lane
//   checks 5..8  `in` is an LDS image of n_in_bytes (a multiple of 4, at most
//                2048); `addr` the 64 per-lane byte offsets, 8-byte aligned
//                and in bounds
//   check 9      `in` is a global image of n_in_bytes (at most 8192); `addr`
//                the 64 per-lane byte offsets, aligned to the size and, with
//                the instruction offset, in bounds; `out` is the data
//                registers, then the guard register
// 0 ok, -10 bad argument, -1 HIP error.
int cro_movement_tile(int device, int test, int variant, const void* in, int n_in_bytes,
                      const int* addr, void* out, int n_out_bytes);

#ifdef __cplusplus
}
#endif
