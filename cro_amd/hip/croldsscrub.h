// C ABI of libcroldsscrub.so (ldsscrub.hip): clear and verify every CU's LDS
// before a device is drained and handed back to the fabric pool.
//
// LDS is 160 KiB on each CU.  It is the on-chip memory a kernel can read
// without ever having written it, and nothing here shows that the hardware or
// the driver clears it between processes; a PCI remove does not power-cycle
// the device.  cro_lds_scrub_run places one 256-thread workgroup on every CU
// (the whole-CU dynamic-LDS request does that, as in the compute-coverage
// stage), and each workgroup counts what it finds (the census), stores one
// fill word everywhere and reads every word back.  A further dispatch (the
// recheck) counts once more: that is what a later kernel would find.
//
// What it does NOT cover: registers.  The vector register file is the
// register scrub stage's (croregscrub.h, regscrub.hip); SGPRs and the
// hardware state registers no stage covers.  Only counts and offsets leave
// the device, never what was found: that is another tenant's data.
//
// Plain C/C++: nodeops/ldsscrub.py mirrors both ABI structs with ctypes (keep
// field order in sync there; tests/test_lds_scrub.py compares
// sizeof/offsetof), croagent takes cro_lds_scrub_run by dlsym, and a host
// compiler without HIP can include this file.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "crocoverage.h"  // cro_cov_cu_key, cro_cov_decode

enum {
  CRO_LDS_SCRUB_BYTES = 163840,           // one CU's whole LDS
  CRO_LDS_SCRUB_WORDS = 163840 / 4
};
// self-test: preset of the words that are not marched
#define CRO_LDS_SCRUB_GUARD_WORD 0xA5A5A5A5u

#ifdef __cplusplus
extern "C" {
#endif

struct CroLdsScrubOpts {
  int lds_bytes;   // marched per workgroup: a multiple of 16, at most 163840; 0 = all
  int grid;        // workgroups per dispatch; 0 = multiProcessorCount
  int max_rounds;  // dispatches while some CU is unseen; 0 = 4, at most 64
  int skip_recheck;  // non-zero: no census-only dispatch after the last round
  unsigned int fill_word;  // default 0
  // Self-test, for tests only (0 = off); through data alone, in bounds, inside
  // the kernel, every plant stored by another thread than the one that reads
  // the word later.  In every mode the words from lds_bytes / 4 to the end of
  // the LDS are preset to the guard word and counted in guard_bad when they
  // changed.  fill_word and selftest_pattern must differ from the guard word
  // and from each other.
  //   1: selftest_pattern planted in every marched word, then a normal run
  //   2: fill_word planted in every marched word and selftest_pattern in word
  //      selftest_word, then a normal run
  //   3: as 1, but the fill is skipped
  //   4: a normal run, but bit selftest_bit of word selftest_word is flipped
  //      between fill and verify
  int selftest_mode;
  unsigned int selftest_pattern;
  unsigned int selftest_word;  // below lds_bytes / 4
  int selftest_bit;            // 0..31
  int reserved;
  double min_cu_fraction;  // 0 = off; else fail when cus_seen / cus_expected is below
};

struct CroLdsScrubResult {
  int ok;
  int rc;  // 0 ok, -1 HIP error or bad argument, -42 LDS residue, -43 coverage below floor
  int cus_expected;  // multiProcessorCount
  int cus_seen;      // distinct (XCD, SE, SH, CU) a scrubbing workgroup ran on
  int xcds_seen;
  int rounds;
  int lds_bytes;  // marched per workgroup
  int grid;
  unsigned long long workgroups;          // of all rounds (the recheck's are not counted)
  unsigned long long bytes_scrubbed;      // workgroups x lds_bytes; 0 when the fill was skipped
  unsigned long long dirty_words_before;  // census: words != fill_word as found
  unsigned long long dirty_workgroups;    // workgroups whose census found any
  unsigned long long n_bad;               // words != fill_word after the fill
  unsigned long long guard_bad;           // self-test: guard words that changed
  unsigned long long recheck_dirty_words;  // census of the recheck dispatch
  unsigned int first_dirty_word;  // lowest word offset in a workgroup's LDS; ~0 = none
  unsigned int first_bad_word;    // of the first bad workgroup; ~0 = none
  unsigned int bits_bad;          // OR of got ^ fill_word over all bad words
  int bad_workgroups;
  // where the first bad workgroup ran (lowest record index, the recheck's
  // records after the rounds'); -1 when there is none
  int xcd, se, sh, cu;
  double gpu_ms;  // event-timed, all dispatches
  double t_total_ms;
  char msg[256];
};

int cro_lds_scrub_run(int device, const struct CroLdsScrubOpts* opts,
                      struct CroLdsScrubResult* out);
// The same, and the rounds' records (below) in dispatch order, at most
// max_records of them: rounds x grid were written.  For tests.
struct CroLdsScrubRecord;
int cro_lds_scrub_run_records(int device, const struct CroLdsScrubOpts* opts,
                              struct CroLdsScrubResult* out,
                              struct CroLdsScrubRecord* records_out, int max_records);

#ifdef __cplusplus
}
#endif

// -- record -----------------------------------------------------------------------

// One per workgroup and dispatch, preset by the host (CRO_LDS_SCRUB_CLEAN_RECORD);
// a wave adds to it with atomics only when it has something to add, lane 0 of
// wave 0 writes where the workgroup ran.  Offsets are 32-bit words from the
// start of the workgroup's LDS.
struct CroLdsScrubRecord {
  uint32_t xcc_id;       // raw XCC_ID register
  uint32_t hw_id;        // raw HW_ID register
  uint32_t dirty_words;  // census
  uint32_t first_dirty;  // ~0 = none
  uint32_t n_bad;        // verify
  uint32_t first_bad;    // ~0 = none
  uint32_t bits_bad;
  uint32_t guard_bad;
  uint32_t valid;  // 1 once the workgroup wrote the record
  uint32_t reserved;
};

#define CRO_LDS_SCRUB_CLEAN_RECORD {0u, 0u, 0u, ~0u, 0u, ~0u, 0u, 0u, 0u, 0u}

// -- aggregation --------------------------------------------------------------------

struct CroLdsScrubAgg {
  unsigned long long workgroups;  // valid records
  unsigned long long dirty_words;
  unsigned long long dirty_workgroups;
  unsigned long long n_bad;
  unsigned long long bad_workgroups;  // records with bad or changed guard words
  unsigned long long guard_bad;
  long long first_bad_index;  // index of the first record with n_bad != 0; -1 = none
  int cus_seen;               // distinct CU keys
  int xcds_seen;
  int xcd, se, sh, cu;  // of that record; -1 when there is none
  unsigned int first_dirty_word;  // lowest over all records; ~0 = none
  unsigned int first_bad_word;    // of that record; ~0 = none
  unsigned int bits_bad;          // OR over all records
};

// Deterministic: one pass in record order; invalid records are skipped.
static inline void cro_lds_scrub_aggregate(const CroLdsScrubRecord* records, size_t n,
                                           CroLdsScrubAgg* out) {
  // compact key: xcd(4) | se(3) | sh(1) | cu(4) = 12 bits
  unsigned char cus[1 << 12];
  unsigned char xcds[16];
  memset(cus, 0, sizeof(cus));
  memset(xcds, 0, sizeof(xcds));
  memset(out, 0, sizeof(*out));
  out->first_bad_index = -1;
  out->xcd = out->se = out->sh = out->cu = -1;
  out->first_dirty_word = out->first_bad_word = ~0u;
  for (size_t i = 0; i < n; ++i) {
    const CroLdsScrubRecord& r = records[i];
    if (!r.valid) continue;
    ++out->workgroups;
    const unsigned key = cro_cov_cu_key(r.xcc_id, r.hw_id);
    const unsigned idx = ((key >> 16) << 8) | ((key >> 8) & 0xFFu);
    if (!cus[idx]) ++out->cus_seen;
    cus[idx] = 1;
    if (!xcds[key >> 16]) ++out->xcds_seen;
    xcds[key >> 16] = 1;
    if (r.dirty_words) {
      out->dirty_words += r.dirty_words;
      ++out->dirty_workgroups;
      if (r.first_dirty < out->first_dirty_word) out->first_dirty_word = r.first_dirty;
    }
    out->guard_bad += r.guard_bad;
    if (r.n_bad || r.guard_bad) ++out->bad_workgroups;
    if (!r.n_bad) continue;
    out->n_bad += r.n_bad;
    out->bits_bad |= r.bits_bad;
    if (out->first_bad_index < 0) {
      const CroCoverageLoc loc = cro_cov_decode(r.xcc_id, r.hw_id);
      out->first_bad_index = (long long)i;
      out->xcd = (int)loc.xcd;
      out->se = (int)loc.se;
      out->sh = (int)loc.sh;
      out->cu = (int)loc.cu;
      out->first_bad_word = r.first_bad;
    }
  }
}
