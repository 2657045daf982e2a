// Host-only pieces of the deep (data-integrity) probe: the report the verify
// kernel and the host verify fill in, the host side of the link stages, how
// the sizes of a run are normalised, how the VRAM span is cut into chunks and
// which seed and polarity each stage holds.
//
// Plain C++: a host compiler without HIP can include it, so
// tests/test_probe_integrity.py compiles it into a small program of its own.
// integrity.hip is the one user in the library; nothing here is exported.
#pragma once

#include <stdint.h>

#include "cropattern.h"

namespace crointegrity {

struct PatternReport {
  unsigned long long n_bad;
  unsigned long long first_bad;  // global word index, all-ones = none
  unsigned int bits_bad;
  unsigned int pad;
};

inline void host_fill(uint32_t* dst, uint64_t n_words, uint32_t seed, uint32_t invert) {
  for (uint64_t w = 0; w < n_words; ++w) dst[w] = cro_pattern_word(w, seed, invert);
}

inline PatternReport host_verify(const uint32_t* src, uint64_t n_words, uint32_t seed,
                                 uint32_t invert) {
  PatternReport r = {0, ~0ull, 0, 0};
  for (uint64_t w = 0; w < n_words; ++w) {
    const uint32_t d = src[w] ^ cro_pattern_word(w, seed, invert);
    if (d) {
      if (r.n_bad == 0) r.first_bad = w;
      ++r.n_bad;
      r.bits_bad |= d;
    }
  }
  return r;
}

// -- sizes ---------------------------------------------------------------------

constexpr long long kGiB = 1ll << 30;
constexpr long long kDefaultVramBytes = kGiB;
constexpr long long kDefaultLinkBytes = 256ll << 20;
constexpr long long kMaxChunkBytes = kGiB;

struct Sizes {
  uint64_t vram_words;   // whole words only: bytes >> 2
  uint64_t link_words;
  uint64_t chunk_words;  // a multiple of 4 (whole 16-byte vectors), 4 .. 2^28
};

// Options as the caller gave them (0 or negative = default) to what a run uses.
inline Sizes normalise_sizes(long long vram_bytes, long long link_bytes, long long chunk_bytes) {
  if (vram_bytes <= 0) vram_bytes = kDefaultVramBytes;
  if (link_bytes <= 0) link_bytes = kDefaultLinkBytes;
  if (chunk_bytes <= 0 || chunk_bytes > kMaxChunkBytes) chunk_bytes = kMaxChunkBytes;
  chunk_bytes &= ~15ll;  // every chunk but the last holds whole 16-byte vectors
  if (chunk_bytes < 16) chunk_bytes = 16;
  Sizes s;
  s.vram_words = (uint64_t)vram_bytes >> 2;
  s.link_words = (uint64_t)link_bytes >> 2;
  s.chunk_words = (uint64_t)chunk_bytes >> 2;
  return s;
}

// -- chunk plan ------------------------------------------------------------------

// The VRAM span as a list of chunks: count() of them, chunk c holding words(c)
// words that start at word base(c) of the span.  Every chunk but the last has
// chunk_words; the last has what is left (1 .. chunk_words).
struct ChunkPlan {
  uint64_t span_words;
  uint64_t chunk_words;

  uint64_t count() const { return (span_words + chunk_words - 1) / chunk_words; }
  uint64_t base(uint64_t c) const { return c * chunk_words; }
  uint64_t words(uint64_t c) const {
    const uint64_t left = span_words - base(c);
    return left < chunk_words ? left : chunk_words;
  }
};

inline ChunkPlan chunk_plan(uint64_t span_words, uint64_t chunk_words) {
  ChunkPlan p = {span_words, chunk_words};
  return p;
}

struct ChunkPos {
  uint64_t chunk;
  uint64_t word;  // within the chunk
};

// Word `span_word` of the span (below span_words) as chunk and word within it.
inline ChunkPos locate(const ChunkPlan& plan, uint64_t span_word) {
  ChunkPos pos = {span_word / plan.chunk_words, span_word % plan.chunk_words};
  return pos;
}

// -- stages ------------------------------------------------------------------------

// In the order of CroIntegrityOpts::selftest_stage - 1 and of the result's
// per-stage fields.
enum Stage { kVram = 0, kH2dDma, kD2hDma, kH2dKernel, kD2hKernel, kNumStages };

struct StageInfo {
  const char* name;
  uint32_t seed_xor;  // the device→host stages run on seed ^ 0xA5A5A5A5, so a
                      // stale host→device image can never pass
  uint32_t invert;    // the shader stages hold the complement
};

constexpr StageInfo kStages[kNumStages] = {
    {"vram", 0u, 0u},
    {"h2d_dma", 0u, 0u},
    {"d2h_dma", 0xA5A5A5A5u, 0u},
    {"h2d_kernel", 0u, 1u},
    {"d2h_kernel", 0xA5A5A5A5u, 1u},
};

struct StagePattern {
  uint32_t seed;
  uint32_t invert;
};

// What a stage fills and verifies with under the run's seed.  `pass` is the
// VRAM stage's: 0 the pattern, 1 its complement; 0 for a link stage.
inline StagePattern stage_pattern(int stage, uint32_t pass, uint32_t seed) {
  StagePattern p = {seed ^ kStages[stage].seed_xor, kStages[stage].invert ^ (pass & 1u)};
  return p;
}

inline uint64_t stage_span_words(int stage, const Sizes& s) {
  return stage == kVram ? s.vram_words : s.link_words;
}

}  // namespace crointegrity
