// Shared C ABI for the gfx950 health probe library (libcroprobe.so).
// Consumers: probe.hip, integrity.hip and coverage.hip (implementation; their
// shared internals are in crohost.h and cromfma.h, which nothing else includes;
// integrity.hip's host-only pieces are in crointegrity.h),
// agent/croagent.cpp (native CLI),
// nodeops/probe.py (ctypes — keep CroProbeResult field order in sync there).
#pragma once

#include "crocoverage.h"

#ifdef __cplusplus
extern "C" {
#endif

struct CroProbeResult {
  int ok;
  int mfma_f32_exact;  // 1 = bitwise match vs host fmaf chain
  double hbm_gbps;     // achieved copy bandwidth (read+write bytes)
  double bf16_tflops;  // dense bf16 MFMA issue rate
  long long vram_total;
  long long vram_free;
  double t_setup_ms;  // host wall from the entry to the first enqueue
  double t_mfma_ms;   // device time of each section, from the events around it:
  double t_bw_ms;     // the probe is one submission with one wait, so there is
  double t_bf16_ms;   // no host wall per section (attach-latency budget)
  char gcn_arch[64];
  char msg[256];
};

// nodeops/probe.py mirrors CroProbeResult and CroProbeOpts with ctypes
// (tests/test_probe_quick.py compares sizeof/offsetof).
struct CroProbeOpts {
  double hbm_floor_gbps;     // 0 → 500
  double bf16_floor_tflops;  // 0 → 100
  // Self-test, for tests only.  Mode 1: the host flips bit selftest_bit of
  // element selftest_elem (row * 16 + col, below 256) of the EXPECTED f32 tile
  // before the compare, so the exact gate fires through data alone.
  int selftest_mode;
  int selftest_bit;
  unsigned int selftest_elem;
  int reserved;
};

// rc 0 ok, -1 HIP error or bad argument, then in this order: -2 f32 MFMA
// mismatch, -3 HBM bandwidth below its floor, -4 bf16 rate below its floor.
int cro_probe_run(int device, struct CroProbeResult* out);  // = run_opts(device, NULL, out)
int cro_probe_run_opts(int device, const struct CroProbeOpts* opts, struct CroProbeResult* out);

// Lengths of the probe's two rate windows; 0 takes the library default, which
// is what cro_probe_run_opts runs at (profiles/quick_probe_windows_mi355x.md
// has the sweep behind the defaults).  nodeops/probe.py mirrors the struct
// (tests/test_probe_windows.py compares sizeof/offsetof).
struct CroProbeWindows {
  int copy_launches;  // launches of the 2 x 256 MiB copy; at most 64
  int bf16_iters;     // iterations of the rate kernel; at most 65536
  // Test seam: 1 leaves the check kernel out, so the exact gate sees the
  // tile as the in-stream poison left it and must fail with rc -2.
  int skip_check_launch;
  int reserved;
};

// The probe's pipeline at these windows (NULL: the defaults), floors at their
// defaults; rc as cro_probe_run_opts.  A negative field or one above its
// limit is a bad argument.
int cro_probe_run_windows(int device, const struct CroProbeWindows* w,
                          struct CroProbeResult* out);
// Raw entries for tests, one per kernel of the quick probe (probe.hip).
// -10 = bad argument.  K a multiple of 4, at most 4096.
int cro_probe_mfma_f32(int device, const float* A, const float* B, float* D, int K);
// bw_copy_kernel over n4 16-byte vectors with grid_blocks x 256 threads;
// *guard_ok = the 64 vectors after dst untouched; -11 = src was changed.
int cro_probe_copy(int device, const void* src_host, unsigned long long n4, int grid_blocks,
                   void* dst_host, int* guard_ok);
// The probe's own copy launch on its cached buffers, dst zeroed first: the
// bytes of dst that are not 0x5a afterwards.
int cro_probe_bw_selfcheck(int device, unsigned long long* n_bad,
                           unsigned long long* first_bad);
// mfma_bf16_rate_kernel; out_host gets blocks floats, or blocks * 256 with all_lanes.
int cro_probe_bf16_sink(int device, int blocks, int iters, int all_lanes, float* out_host);
void* cro_probe_alloc(int device, long long bytes);
void cro_probe_free(void* p);
int cro_probe_device_count(void);
int cro_probe_pci_bus_id(int device, char* buf, int len);

// -- deep probe: data integrity of VRAM and of the host link (integrity.hip).
// nodeops/probe.py mirrors both structs with ctypes — keep field order in
// sync there (tests/test_probe_integrity.py compares sizeof/offsetof).

struct CroIntegrityOpts {
  long long vram_bytes;    // 0 → library default (1 GiB)
  long long link_bytes;    // 0 → library default (256 MiB)
  long long chunk_bytes;   // VRAM allocation unit; 0 or > 1 GiB → 1 GiB
  unsigned int seed;       // 0 is a valid seed
  // Self-test, for tests only (all zero = off): in stage selftest_stage (1 vram,
  // 2 h2d_dma, 3 d2h_dma, 4 h2d_kernel, 5 d2h_kernel) the host flips bit
  // selftest_bit of word selftest_word of the stage's span after the stage's
  // data is written and before it is verified, so the stage must detect,
  // locate and report through data alone.  Every access is in bounds.
  int selftest_stage;
  double link_floor_gbps;  // 0 = off; else every link rate must reach it
  int selftest_pass;       // vram only: 0 the pattern pass, 1 the complement pass
  int selftest_bit;        // 0..31
  unsigned long long selftest_word;  // below the stage's span in words
};

struct CroIntegrityResult {
  int ok;
  int rc;  // 0 ok, -1 HIP error or bad argument, -20 data mismatch, -21 link floor
  unsigned long long n_bad;           // of the failing stage (0 when ok)
  unsigned long long first_bad_byte;  // byte offset in the stage's span; ~0 = none
  unsigned int bits_bad;              // OR of got ^ want over the bad words
  int vram_passes;                    // pattern then inverted pattern = 2
  int link_passes;
  int vram_chunks;
  // bytes whose content was compared, summed over passes
  long long vram_bytes_verified;
  long long h2d_dma_bytes_verified;
  long long d2h_dma_bytes_verified;
  long long h2d_kernel_bytes_verified;
  long long d2h_kernel_bytes_verified;
  unsigned long long vram_n_bad;
  unsigned long long h2d_dma_n_bad;
  unsigned long long d2h_dma_n_bad;
  unsigned long long h2d_kernel_n_bad;
  unsigned long long d2h_kernel_n_bad;
  // event-timed rates, reported and (but for link_floor_gbps) not gated
  double vram_fill_gbps;
  double vram_verify_gbps;
  double h2d_dma_gbps;
  double d2h_dma_gbps;
  double h2d_kernel_gbps;
  double d2h_kernel_gbps;
  double t_vram_ms;  // host wall per stage, allocation and host work included
  double t_link_dma_ms;
  double t_link_kernel_ms;
  double t_total_ms;
  char failed_stage[32];  // "", "vram", "h2d_dma", "d2h_dma", "h2d_kernel", "d2h_kernel"
  char msg[256];
  unsigned int first_bad_got;  // the word found at first_bad_byte; 0 when none
  int reserved;
};

int cro_probe_integrity(int device, const struct CroIntegrityOpts* opts,
                        struct CroIntegrityResult* out);
// Raw kernel entries for tests: fill on the device and copy back / upload a
// host buffer and verify it on the device.  The device buffer is followed by
// 64 guard vectors; they and the 0-3 slack words after n_words are preset to
// 0xA5 bytes.  *guard_ok = the fill left all of them untouched; a verify that
// read one of them would report a mismatch.
int cro_probe_pattern_fill(int device, unsigned int seed, int invert,
                           unsigned long long base_word, unsigned long long n_words,
                           unsigned int* host_out, int* guard_ok);
int cro_probe_pattern_verify(int device, unsigned int seed, int invert,
                             unsigned long long base_word, unsigned long long n_words,
                             const unsigned int* host_in, unsigned long long* n_bad,
                             unsigned long long* first_bad, unsigned int* bits_bad);

// -- compute-coverage stage: exact checks on every CU and SIMD, with fault
// location (coverage.hip; record, decode and aggregate in crocoverage.h).
// nodeops/probe.py mirrors both structs with ctypes — keep field order in
// sync there (tests/test_probe_compute.py compares sizeof/offsetof).

struct CroComputeOpts {
  int grid_blocks;  // 0 → multiProcessorCount
  int lds_bytes;    // 0 → 163840 (a CU's whole LDS: one workgroup per CU);
                    // a multiple of 16, at most 163840
  int iters;        // 0 → 16 (≈0.6 ms; profiles/compute_probe_mi355x.md); repeats
                    // of all four checks per wave
  int max_rounds;   // 0 → 4; launches while some CU or SIMD is still unseen
  unsigned int seed;  // 0 is a valid seed
  // Self-test, for tests only: shows detection and localisation through data
  // alone.  Mode 1: the host flips bit selftest_bit of element selftest_elem
  // in the EXPECTED tile of test selftest_test (0 f32, 1 i8, 2 bf16, 3 LDS)
  // before upload; every wave must flag it.  Mode 2: the kernel flips that
  // bit in its COMPUTED value on the waves whose CU key is selftest_key;
  // exactly those waves may flag it.  For the LDS test, where each word is
  // checked by one wave only, the flip is repeated at the same lane and trip
  // of all four waves of a workgroup.  Neither mode makes an LDS word wrong:
  // for the LDS test both alter a difference already in a register.
  // Modes 3 and 4 (selftest_test = 3 only) plant in LDS itself: in the passes
  // selftest_pass names, of every iteration, after the fill's barrier and
  // before the verify loads, the kernel flips bit selftest_bit of the
  // selftest_span words from selftest_elem on with real LDS stores, each word
  // by a thread of another wave than the one that verifies it, then takes a
  // second barrier.  The verify loop is the clean run's.  Mode 3: on every
  // workgroup.  Mode 4: on the workgroups whose CU key is selftest_key.  All
  // stores are in bounds: wrong data only.
  int selftest_mode;
  int selftest_test;
  int selftest_bit;
  unsigned int selftest_elem;
  unsigned int selftest_key;
  unsigned int selftest_span;  // modes 3, 4: words, >= 1, elem + span <= lds_bytes / 4
  int selftest_pass;           // modes 3, 4: 0 pattern, 1 complement, 2 both
  double min_cu_fraction;  // 0 = off; else fail when cus_seen / cus_expected is below
};

struct CroComputeResult {
  int ok;
  int rc;  // 0 ok, -1 HIP error or bad argument, -30 compute mismatch, -31 coverage floor
  int cus_expected;  // hipDeviceProp_t::multiProcessorCount
  int rounds;        // launches of the grid
  struct CroCoverageAgg agg;  // over all rounds
  int first_bad_round;   // of the first bad wave; -1 = none
  int first_bad_record;  // workgroup * 4 + wave within that round; -1 = none
  int grid_blocks;       // as run
  int lds_bytes;
  int iters;
  int reserved;
  double gpu_ms;      // event-timed, summed over the rounds
  double t_total_ms;  // host wall
  char failed_test[16];  // "", "mfma_f32", "mfma_i8", "mfma_bf16", "lds"
  char msg[256];
};

int cro_probe_compute(int device, const struct CroComputeOpts* opts,
                      struct CroComputeResult* out);
// The same, and copies out the raw records (rounds * grid_blocks * 4 of them,
// round-major) up to max_records, for tests.
int cro_probe_compute_records(int device, const struct CroComputeOpts* opts,
                              struct CroComputeResult* out,
                              struct CroCoverageRecord* records_out, int max_records);
// The same, with the caller's expected tiles, for tests of the per-wave
// tallies: each non-null tile (e32 256 floats, e8 256 ints, e16 1024 floats,
// row-major) stands in for the cached expected tile in this call only.  The
// kernel is the same; it is handed another pointer.
int cro_probe_compute_tiles(int device, const struct CroComputeOpts* opts, const float* e32,
                            const int* e8, const float* e16, struct CroComputeResult* out,
                            struct CroCoverageRecord* records_out, int max_records);
// Raw entry for tests of the LDS march: the coverage kernel itself (one
// iteration, grid_blocks workgroups, at most 8) up to the fill of pass `pass`
// (0 pattern, 1 complement), its barrier and, with plant_span > 0, a plant as
// self-test mode 3 makes it (plant_elem, plant_span, plant_bit); then each
// workgroup copies its LDS to host_out + workgroup * lds_bytes / 4 and
// returns.  Where lds_bytes <= 163840 - 1024 the launch asks for 1024 bytes
// more, preset to 0xA5A5A5A5 before the fill: *guard_bad_out = how many of
// those 256 words per workgroup changed, summed.  -10 = bad argument.
int cro_probe_compute_lds_dump(int device, int grid_blocks, int lds_bytes, unsigned int seed,
                               int pass, unsigned int plant_elem, unsigned int plant_span,
                               int plant_bit, unsigned int* host_out,
                               unsigned int* guard_bad_out);
// Raw tile entry for the lane-map tests, one wave of the coverage kernel's
// body on caller data.  kind 1: i8, A 16xK, B Kx16 (int8), D 16x16 (int32),
// K a multiple of 64.  kind 2: bf16, A 32xK, B Kx32 (bf16 bit patterns),
// D 32x32 (float), K a multiple of 16.  Row-major; K at most 4096.
int cro_probe_mfma_tile(int device, int kind, const void* A, const void* B, void* D, int K);

#ifdef __cplusplus
}
#endif
