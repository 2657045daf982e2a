// Host-only pieces of the scrub stage: how many bytes a run goes for, how it
// asks the driver for them, and where a word of the concatenated span lies.
//
// Plain C++: a host compiler without HIP can include it, so
// tests/test_scrub.py compiles it into a small program with fake allocators.
// scrub.hip is the one user in the library; nothing here is exported.
#pragma once

#include <stdint.h>

#include <vector>

namespace croscrub {

constexpr uint64_t kAlignBytes = 256;              // every request is a multiple
constexpr uint64_t kFloorBytes = 2ull << 20;       // a refusal at or below ends the plan
constexpr uint64_t kMaxChunkBytes = 1ull << 30;    // and the default
constexpr uint64_t kMinReserveBytes = 256ull << 20;

inline uint64_t align_down(uint64_t bytes) { return bytes & ~(kAlignBytes - 1); }

// Options as the caller gave them to what a run uses.
inline uint64_t normalise_chunk(long long chunk_bytes) {
  if (chunk_bytes <= 0 || (uint64_t)chunk_bytes > kMaxChunkBytes) return kMaxChunkBytes;
  const uint64_t c = align_down((uint64_t)chunk_bytes);
  return c < kAlignBytes ? kAlignBytes : c;
}

// The reserve is a safety condition for the runtime's own allocations, not a
// tuned number: a larger one is honoured, a smaller one is raised.
inline uint64_t normalise_reserve(long long reserve_bytes) {
  if (reserve_bytes <= 0 || (uint64_t)reserve_bytes < kMinReserveBytes) return kMinReserveBytes;
  return (uint64_t)reserve_bytes;
}

// free - reserve, capped by max_bytes when that is positive, whole 256 B.
inline uint64_t target_bytes(uint64_t free_bytes, long long reserve_bytes, long long max_bytes) {
  const uint64_t reserve = normalise_reserve(reserve_bytes);
  if (free_bytes <= reserve) return 0;
  uint64_t target = free_bytes - reserve;
  if (max_bytes > 0 && (uint64_t)max_bytes < target) target = (uint64_t)max_bytes;
  return align_down(target);
}

struct PlanStats {
  uint64_t granted_bytes;
  uint64_t requests;
  uint64_t refusals;
  uint64_t chunks;
};

// Asks try_alloc(bytes) -> bool for `target` bytes (a multiple of 256) in
// requests of `chunk` bytes (normalise_chunk), the last one of what is left.
// A refused request halves the size of the ones after it (whole 256 B); the
// plan ends when a request at or below the floor is refused, or when nothing
// is left.  So a remainder below the floor is asked for once, as it is.
template <class TryAlloc>
PlanStats acquire(uint64_t target, uint64_t chunk, TryAlloc&& try_alloc) {
  PlanStats s = {0, 0, 0, 0};
  uint64_t left = target;
  uint64_t size = chunk;
  while (left >= kAlignBytes && size >= kAlignBytes) {
    const uint64_t ask = size < left ? size : left;
    ++s.requests;
    if (try_alloc(ask)) {
      s.granted_bytes += ask;
      left -= ask;
      ++s.chunks;
      continue;
    }
    ++s.refusals;
    if (ask <= kFloorBytes) break;
    size = align_down(ask / 2);
  }
  return s;
}

// The chunks a run holds, in the order granted, as one span of words.
class ChunkList {
 public:
  void add(uint64_t words) {
    base_.push_back(span_words_);
    words_.push_back(words);
    span_words_ += words;
  }
  uint64_t count() const { return words_.size(); }
  uint64_t span_words() const { return span_words_; }
  uint64_t base(uint64_t c) const { return base_[c]; }    // first span word of chunk c
  uint64_t words(uint64_t c) const { return words_[c]; }

  struct Pos {
    uint64_t chunk;
    uint64_t word;  // within the chunk
  };
  // Word `span_word` (below span_words()) as chunk and word within it.
  Pos locate(uint64_t span_word) const {
    uint64_t lo = 0, hi = words_.size();  // last chunk with base <= span_word
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) / 2;
      if (base_[mid] <= span_word) lo = mid; else hi = mid;
    }
    const Pos pos = {lo, span_word - base_[lo]};
    return pos;
  }

 private:
  std::vector<uint64_t> base_, words_;
  uint64_t span_words_ = 0;
};

}  // namespace croscrub
