// Shared C ABI for the gfx950 health probe library (libcroprobe.so).
// Consumers: probe.hip and integrity.hip (implementation),
// agent/croagent.cpp (native CLI),
// nodeops/probe.py (ctypes — keep CroProbeResult field order in sync there).
#pragma once

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
  double t_setup_ms;  // host wall per probe section (attach-latency budget)
  double t_mfma_ms;
  double t_bw_ms;
  double t_bf16_ms;
  char gcn_arch[64];
  char msg[256];
};

int cro_probe_run(int device, struct CroProbeResult* out);
int cro_probe_mfma_f32(int device, const float* A, const float* B, float* D, int K);
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
  int reserved;
  double link_floor_gbps;  // 0 = off; else every link rate must reach it
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
};

int cro_probe_integrity(int device, const struct CroIntegrityOpts* opts,
                        struct CroIntegrityResult* out);
// Raw kernel entries for tests: fill on the device and copy back / upload a
// host buffer and verify it on the device.
int cro_probe_pattern_fill(int device, unsigned int seed, int invert,
                           unsigned long long base_word, unsigned long long n_words,
                           unsigned int* host_out);
int cro_probe_pattern_verify(int device, unsigned int seed, int invert,
                             unsigned long long base_word, unsigned long long n_words,
                             const unsigned int* host_in, unsigned long long* n_bad,
                             unsigned long long* first_bad, unsigned int* bits_bad);

#ifdef __cplusplus
}
#endif
