// croagent — native node agent CLI for the cro-amd operator.
//
// In cluster mode the controller runs off-node and reaches node hardware by
// exec'ing into the privileged node-agent pod (the role `nvidia-smi` + shell
// pipelines play in the reference, gpus.go:1040-1067).  This binary is what
// that exec invokes: fork-free KFD sysfs enumeration, per-device compute-pid
// attribution, PCI hot-plug, and the gfx950 health probe — each emitting
// JSON on stdout.
//
//   croagent list   [--sysroot /]            GPU inventory (KFD topology)
//   croagent cxl    [--sysroot /]            CXL.mem inventory (/sys/bus/cxl)
//   croagent pids   [--gpu-id N]             KFD compute processes
//   croagent probe  [--device N | --bdf B]   gfx950 MFMA/HBM health probe
//       [--deep [--vram-mib N] [--link-mib N] [--link-floor-gbps X]]
//                                            + VRAM / host-link data integrity
//       [--compute [--compute-min-cu-fraction X]]
//       [--formats [--formats-min-cu-fraction X]]  + the matrix-format stage
//                                            (libcroformats.so, loaded at run time)
//       [--coherence [--coherence-min-cu-fraction X]]  + the coherence stage:
//                                            atomic units and cross-CU visibility
//                                            (libcrocoherence.so, loaded at run time)
//       [--movement [--movement-min-cu-fraction X]]  + the data-movement stage:
//                                            cross-lane, transposed LDS reads, LDS-DMA
//                                            (libcromovement.so, loaded at run time)
//       [--alu [--alu-min-cu-fraction X]]    + the ALU stage: vector and scalar ALUs,
//                                            transcendental consensus
//                                            (libcroalu.so, loaded at run time)
//                                            + exact checks on every CU and SIMD
//   croagent scrub  [--device N | --bdf B]   overwrite and verify VRAM before drain
//       [--max-mib N] [--reserve-mib N] [--min-fraction X]
//                                            (libcroscrub.so, loaded at run time)
//       [--lds [--lds-min-cu-fraction X]]    + clear and verify every CU's LDS
//                                            (libcroldsscrub.so, loaded at run time)
//       [--regs [--regs-min-simd-fraction X]]  + clear and verify every SIMD's
//                                            vector registers
//                                            (libcroregscrub.so, loaded at run time)
//   croagent drain  --bdf 0000:5a:00.0       sysfs PCI remove
//   croagent rescan                          sysfs PCI rescan
//
// Build (cro_amd/hip/build.py):
//   hipcc --offload-arch=gfx950 -O2 croagent.cpp -L../hip -lcroprobe -o croagent

#include <dirent.h>
#include <dlfcn.h>
#include <unistd.h>

#include "../hip/croprobe.h"
#include "../hip/croldsscrub.h"
#include "../hip/croformats.h"
#include "../hip/crocoherence.h"
#include "../hip/cromovement.h"
#include "../hip/croalu.h"
#include "../hip/croregscrub.h"
#include "../hip/croscrub.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

namespace {

std::string g_sysroot = "";

std::string path(const std::string& p) { return g_sysroot + p; }

bool read_file(const std::string& p, std::string* out) {
  std::ifstream f(path(p));
  if (!f) return false;
  std::stringstream ss;
  ss << f.rdbuf();
  *out = ss.str();
  return true;
}

bool write_file(const std::string& p, const std::string& data) {
  std::ofstream f(path(p));
  if (!f) return false;
  f << data;
  return bool(f);
}

std::vector<std::string> list_dir(const std::string& p) {
  std::vector<std::string> names;
  DIR* d = opendir(path(p).c_str());
  if (!d) return names;
  while (dirent* e = readdir(d)) {
    if (strcmp(e->d_name, ".") && strcmp(e->d_name, "..")) names.push_back(e->d_name);
  }
  closedir(d);
  return names;
}

std::map<std::string, unsigned long long> parse_properties(const std::string& text) {
  // values can exceed LLONG_MAX (unique_id is a full 64-bit fuse) — parse
  // per line with strtoull so one wide value cannot abort the whole file
  std::map<std::string, unsigned long long> props;
  std::istringstream in(text);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string key, value;
    if (ls >> key >> value) props[key] = strtoull(value.c_str(), nullptr, 10);
  }
  return props;
}

struct Gpu {
  int kfd_node = 0;
  long long gpu_id = 0;
  unsigned long long unique_id = 0;
  long long render_minor = 0;
  long long gfx_target = 0;
  long long vram_bytes = 0;
  std::string bdf;
  int card_index = -1;
  std::vector<long long> xgmi_peers;
};

std::string bdf_from_location(long long loc, long long domain) {
  char buf[32];
  snprintf(buf, sizeof(buf), "%04llx:%02llx:%02llx.%llx", domain, (loc >> 8) & 0xff,
           (loc >> 3) & 0x1f, loc & 0x7);
  return buf;
}

std::map<std::string, int> drm_cards_by_bdf() {
  std::map<std::string, int> out;
  for (const auto& entry : list_dir("/sys/class/drm")) {
    if (entry.rfind("card", 0) != 0 || entry.size() <= 4) continue;
    bool digits = true;
    for (size_t i = 4; i < entry.size(); ++i) digits &= bool(isdigit(entry[i]));
    if (!digits) continue;
    std::string uevent;
    if (!read_file("/sys/class/drm/" + entry + "/device/uevent", &uevent)) continue;
    std::istringstream in(uevent);
    std::string line;
    while (std::getline(in, line)) {
      const std::string kPrefix = "PCI_SLOT_NAME=";
      if (line.rfind(kPrefix, 0) == 0) out[line.substr(kPrefix.size())] = atoi(entry.c_str() + 4);
    }
  }
  return out;
}

std::vector<Gpu> enumerate_gpus() {
  std::vector<Gpu> gpus;
  auto cards = drm_cards_by_bdf();
  const std::string base = "/sys/class/kfd/kfd/topology/nodes";
  for (const auto& entry : list_dir(base)) {
    std::string props_text;
    if (!read_file(base + "/" + entry + "/properties", &props_text)) continue;
    auto props = parse_properties(props_text);
    if (props["simd_count"] == 0) continue;
    Gpu g;
    g.kfd_node = atoi(entry.c_str());
    g.unique_id = props["unique_id"];
    g.render_minor = (long long)props["drm_render_minor"];
    g.gfx_target = (long long)props["gfx_target_version"];
    g.bdf = bdf_from_location((long long)props["location_id"], (long long)props["domain"]);
    auto card = cards.find(g.bdf);
    if (card != cards.end()) g.card_index = card->second;
    std::string gpu_id_text;
    if (read_file(base + "/" + entry + "/gpu_id", &gpu_id_text)) g.gpu_id = atoll(gpu_id_text.c_str());
    for (const auto& bank : list_dir(base + "/" + entry + "/mem_banks")) {
      std::string btext;
      if (!read_file(base + "/" + entry + "/mem_banks/" + bank + "/properties", &btext)) continue;
      auto bprops = parse_properties(btext);
      if (bprops["heap_type"] == 1 || bprops["heap_type"] == 2) g.vram_bytes += (long long)bprops["size_in_bytes"];
    }
    for (const auto& link : list_dir(base + "/" + entry + "/io_links")) {
      std::string ltext;
      if (!read_file(base + "/" + entry + "/io_links/" + link + "/properties", &ltext)) continue;
      auto lprops = parse_properties(ltext);
      if (lprops["type"] == 11) g.xgmi_peers.push_back((long long)lprops["node_to"]);  // xGMI
    }
    gpus.push_back(g);
  }
  return gpus;
}

std::string device_id(const Gpu& g) {
  char buf[64];
  if (g.unique_id) {
    snprintf(buf, sizeof(buf), "GPU-%016llx", g.unique_id);
    return buf;
  }
  return "GPU-pci-" + g.bdf;
}

int cmd_list() {
  auto gpus = enumerate_gpus();
  printf("{\"gpus\":[");
  for (size_t i = 0; i < gpus.size(); ++i) {
    const Gpu& g = gpus[i];
    printf("%s{\"device_id\":\"%s\",\"kfd_node\":%d,\"gpu_id\":%lld,"
           "\"render_minor\":%lld,\"card_index\":%d,\"pci_bdf\":\"%s\","
           "\"vram_bytes\":%lld,\"gfx_target\":%lld,\"xgmi_peers\":[",
           i ? "," : "", device_id(g).c_str(), g.kfd_node, g.gpu_id,
           g.render_minor, g.card_index, g.bdf.c_str(), g.vram_bytes, g.gfx_target);
    for (size_t j = 0; j < g.xgmi_peers.size(); ++j)
      printf("%s%lld", j ? "," : "", g.xgmi_peers[j]);
    printf("]}");
  }
  printf("]}\n");
  return 0;
}

int cmd_cxl() {
  const std::string base = "/sys/bus/cxl/devices";
  printf("{\"memdevs\":[");
  bool first = true;
  for (const auto& entry : list_dir(base)) {
    if (entry.rfind("mem", 0) != 0 || entry.size() <= 3 || !isdigit(entry[3])) continue;
    std::string text;
    unsigned long long serial = 0, size = 0;
    long long numa = 0;
    if (read_file(base + "/" + entry + "/serial", &text))
      serial = strtoull(text.c_str(), nullptr, 16);
    if (read_file(base + "/" + entry + "/ram/size", &text))
      size = strtoull(text.c_str(), nullptr, 16);
    if (read_file(base + "/" + entry + "/numa_node", &text)) numa = atoll(text.c_str());
    std::string bdf;
    if (read_file(base + "/" + entry + "/device/uevent", &text)) {
      std::istringstream in(text);
      std::string line;
      while (std::getline(in, line)) {
        const std::string kPrefix = "PCI_SLOT_NAME=";
        if (line.rfind(kPrefix, 0) == 0) bdf = line.substr(kPrefix.size());
      }
    }
    char id[64];
    if (serial) snprintf(id, sizeof(id), "CXL-%016llx", serial);
    else snprintf(id, sizeof(id), "CXL-pci-%s", bdf.c_str());
    printf("%s{\"device_id\":\"%s\",\"memdev\":\"%s\",\"size_bytes\":%llu,"
           "\"numa_node\":%lld,\"pci_bdf\":\"%s\"}",
           first ? "" : ",", id, entry.c_str(), size, numa, bdf.c_str());
    first = false;
  }
  printf("]}\n");
  return 0;
}

int cmd_pids(long long gpu_id) {
  const std::string base = "/sys/class/kfd/kfd/proc";
  printf("{\"pids\":[");
  bool first = true;
  for (const auto& entry : list_dir(base)) {
    if (entry.empty() || !isdigit(entry[0])) continue;
    if (gpu_id >= 0) {
      std::string vram;
      char fname[64];
      snprintf(fname, sizeof(fname), "/vram_%lld", gpu_id);
      if (!read_file(base + "/" + entry + fname, &vram)) continue;
      if (atoll(vram.c_str()) <= 0) continue;
    }
    printf("%s%s", first ? "" : ",", entry.c_str());
    first = false;
  }
  printf("]}\n");
  return 0;
}

int cmd_drain(const std::string& bdf) {
  if (bdf.empty()) {
    fprintf(stderr, "drain requires --bdf\n");
    return 2;
  }
  if (!write_file("/sys/bus/pci/devices/" + bdf + "/remove", "1")) {
    fprintf(stderr, "failed to write pci remove for %s\n", bdf.c_str());
    return 1;
  }
  printf("{\"drained\":\"%s\"}\n", bdf.c_str());
  return 0;
}

int cmd_rescan() {
  if (!write_file("/sys/bus/pci/rescan", "1")) {
    fprintf(stderr, "failed to write pci rescan\n");
    return 1;
  }
  printf("{\"rescanned\":true}\n");
  return 0;
}

int resolve_device_by_bdf(const std::string& bdf) {
  int count = cro_probe_device_count();
  char buf[64];
  std::string want = bdf.substr(0, bdf.rfind('.'));  // match domain:bus:dev
  for (int dev = 0; dev < count; ++dev) {
    if (cro_probe_pci_bus_id(dev, buf, sizeof(buf)) == 0) {
      std::string got(buf);
      for (auto& c : got) c = tolower(c);
      if (got.rfind(want, 0) == 0) return dev;
    }
  }
  return -1;
}

void print_integrity(const CroIntegrityResult& r) {
  printf("\"integrity\":{\"ok\":%s,\"rc\":%d,\"n_bad\":%llu,\"first_bad_byte\":%llu,"
         "\"bits_bad\":%u,\"first_bad_got\":%u,\"failed_stage\":\"%s\",\"vram_passes\":%d,"
         "\"link_passes\":%d,\"vram_chunks\":%d,",
         r.ok ? "true" : "false", r.rc, r.n_bad, r.first_bad_byte, r.bits_bad, r.first_bad_got,
         r.failed_stage, r.vram_passes, r.link_passes, r.vram_chunks);
  printf("\"vram_bytes_verified\":%lld,\"h2d_dma_bytes_verified\":%lld,"
         "\"d2h_dma_bytes_verified\":%lld,\"h2d_kernel_bytes_verified\":%lld,"
         "\"d2h_kernel_bytes_verified\":%lld,",
         r.vram_bytes_verified, r.h2d_dma_bytes_verified, r.d2h_dma_bytes_verified,
         r.h2d_kernel_bytes_verified, r.d2h_kernel_bytes_verified);
  printf("\"vram_n_bad\":%llu,\"h2d_dma_n_bad\":%llu,\"d2h_dma_n_bad\":%llu,"
         "\"h2d_kernel_n_bad\":%llu,\"d2h_kernel_n_bad\":%llu,",
         r.vram_n_bad, r.h2d_dma_n_bad, r.d2h_dma_n_bad, r.h2d_kernel_n_bad,
         r.d2h_kernel_n_bad);
  printf("\"vram_fill_gbps\":%.1f,\"vram_verify_gbps\":%.1f,\"h2d_dma_gbps\":%.1f,"
         "\"d2h_dma_gbps\":%.1f,\"h2d_kernel_gbps\":%.1f,\"d2h_kernel_gbps\":%.1f,",
         r.vram_fill_gbps, r.vram_verify_gbps, r.h2d_dma_gbps, r.d2h_dma_gbps,
         r.h2d_kernel_gbps, r.d2h_kernel_gbps);
  printf("\"t_vram_ms\":%.1f,\"t_link_dma_ms\":%.1f,\"t_link_kernel_ms\":%.1f,"
         "\"t_total_ms\":%.1f,\"msg\":\"%s\"}",
         r.t_vram_ms, r.t_link_dma_ms, r.t_link_kernel_ms, r.t_total_ms, r.msg);
}

void print_compute(const CroComputeResult& r) {
  const CroCoverageAgg& a = r.agg;
  printf("\"compute\":{\"ok\":%s,\"rc\":%d,\"cus_expected\":%d,\"rounds\":%d,"
         "\"waves_run\":%llu,\"waves_bad\":%llu,\"bad_f32\":%llu,\"bad_i8\":%llu,"
         "\"bad_bf16\":%llu,\"bad_lds\":%llu,\"first_bad_index\":%lld,",
         r.ok ? "true" : "false", r.rc, r.cus_expected, r.rounds, a.waves_run, a.waves_bad,
         a.bad_f32, a.bad_i8, a.bad_bf16, a.bad_lds, a.first_bad_index);
  printf("\"cus_seen\":%d,\"xcds_seen\":%d,\"simds_seen\":%d,\"cus_bad\":%d,\"xcd\":%d,"
         "\"se\":%d,\"sh\":%d,\"cu\":%d,\"simd\":%d,\"first_fail_mask\":%u,\"n_bad\":%u,"
         "\"first_bad\":%u,\"bits_bad\":%u,\"n_bad_cu_keys\":%d,\"bad_cu_keys\":[",
         a.cus_seen, a.xcds_seen, a.simds_seen, a.cus_bad, a.xcd, a.se, a.sh, a.cu, a.simd,
         a.first_fail_mask, a.n_bad, a.first_bad, a.bits_bad, a.n_bad_cu_keys);
  for (int i = 0; i < a.n_bad_cu_keys; ++i) printf("%s%u", i ? "," : "", a.bad_cu_keys[i]);
  printf("],\"first_bad_round\":%d,\"first_bad_record\":%d,\"grid_blocks\":%d,"
         "\"lds_bytes\":%d,\"iters\":%d,\"gpu_ms\":%.3f,\"t_total_ms\":%.3f,"
         "\"failed_test\":\"%s\",\"msg\":\"%s\"}",
         r.first_bad_round, r.first_bad_record, r.grid_blocks, r.lds_bytes, r.iters, r.gpu_ms,
         r.t_total_ms, r.failed_test, r.msg);
}

// The matrix-format stage's result, keys as nodeops/formats.py run_formats.
void print_formats(const CroFormatsResult& r) {
  const CroFormatsAgg& a = r.agg;
  printf("\"formats\":{\"ok\":%s,\"rc\":%d,\"cus_expected\":%d,\"rounds\":%d,"
         "\"waves_run\":%llu,\"waves_bad\":%llu,",
         r.ok ? "true" : "false", r.rc, r.cus_expected, r.rounds, a.waves_run, a.waves_bad);
  for (int t = 0; t < CRO_FMT_TESTS; ++t)
    printf("\"bad_%s\":%llu,", cro_fmt_test(t)->name, a.bad[t]);
  printf("\"first_bad_index\":%lld,\"cus_seen\":%d,\"xcds_seen\":%d,\"simds_seen\":%d,"
         "\"cus_bad\":%d,\"xcd\":%d,\"se\":%d,\"sh\":%d,\"cu\":%d,\"simd\":%d,"
         "\"first_fail_mask\":%u,\"n_bad\":%u,\"first_bad\":%u,\"bits_bad\":%u,",
         a.first_bad_index, a.cus_seen, a.xcds_seen, a.simds_seen, a.cus_bad, a.xcd, a.se, a.sh,
         a.cu, a.simd, a.first_fail_mask, a.n_bad, a.first_bad, a.bits_bad);
  printf("\"first_bad_round\":%d,\"first_bad_record\":%d,\"grid_blocks\":%d,\"iters\":%d,"
         "\"gpu_ms\":%.3f,\"t_total_ms\":%.3f,\"failed_test\":\"%s\",\"msg\":\"%s\"}",
         r.first_bad_round, r.first_bad_record, r.grid_blocks, r.iters, r.gpu_ms, r.t_total_ms,
         r.failed_test, r.msg);
}

// The coherence stage's result, keys as nodeops/coherence.py run_coherence.
void print_coherence(const CroCoherenceResult& r) {
  const CroCoherenceAgg& a = r.agg;
  printf("\"coherence\":{\"ok\":%s,\"rc\":%d,\"cus_expected\":%d,\"rounds\":%d,"
         "\"waves_run\":%llu,\"waves_bad\":%llu,",
         r.ok ? "true" : "false", r.rc, r.cus_expected, r.rounds, a.waves_run, a.waves_bad);
  for (int t = 0; t < CRO_COH_TESTS; ++t) printf("\"bad_%s\":%llu,", kCroCohTestNames[t], a.bad[t]);
  printf("\"pairs_checked\":%llu,\"pairs_expected\":%llu,\"vis_bad\":%llu,\"vis_stale\":%llu,"
         "\"tally_got\":%llu,\"tally_want\":%llu,\"first_bad_index\":%lld,\"cus_seen\":%d,"
         "\"xcds_seen\":%d,\"simds_seen\":%d,\"cus_bad\":%d,\"xcd\":%d,\"se\":%d,\"sh\":%d,"
         "\"cu\":%d,\"simd\":%d,\"fail_mask\":%u,\"first_fail_mask\":%u,\"n_bad\":%u,"
         "\"first_bad\":%u,\"bits_bad\":%u,\"tally_level\":%d,\"tally_slot\":%d,"
         "\"tally_unit\":%d,\"tally_epoch\":%d,\"bad_block\":%d,\"ticket_slot\":%d,"
         "\"ticket_epoch\":%d,\"ticket_seen\":%u,\"ticket_owner\":%u,",
         a.pairs_checked, a.pairs_expected, a.vis_bad, a.vis_stale, a.tally_got, a.tally_want,
         a.first_bad_index, a.cus_seen, a.xcds_seen, a.simds_seen, a.cus_bad, a.xcd, a.se, a.sh,
         a.cu, a.simd, a.fail_mask, a.first_fail_mask, a.n_bad, a.first_bad, a.bits_bad,
         a.tally_level, a.tally_slot, a.tally_unit, a.tally_epoch, a.bad_block, a.ticket_slot,
         a.ticket_epoch, a.ticket_seen, a.ticket_owner);
  printf("\"first_bad_round\":%d,\"first_bad_record\":%d,\"grid_blocks\":%d,\"iters\":%d,"
         "\"gpu_ms\":%.3f,\"t_total_ms\":%.3f,\"failed_test\":\"%s\",\"msg\":\"%s\"}",
         r.first_bad_round, r.first_bad_record, r.grid_blocks, r.iters, r.gpu_ms, r.t_total_ms,
         r.failed_test, r.msg);
}

// The data-movement stage's result, keys as nodeops/movement.py run_movement.
void print_movement(const CroMovementResult& r) {
  const CroMovementAgg& a = r.agg;
  printf("\"movement\":{\"ok\":%s,\"rc\":%d,\"cus_expected\":%d,\"rounds\":%d,"
         "\"waves_run\":%llu,\"waves_bad\":%llu,",
         r.ok ? "true" : "false", r.rc, r.cus_expected, r.rounds, a.waves_run, a.waves_bad);
  for (int t = 0; t < CRO_MOV_TESTS; ++t) printf("\"bad_%s\":%llu,", kCroMovTestNames[t], a.bad[t]);
  printf("\"cus_seen\":%d,\"xcds_seen\":%d,\"simds_seen\":%d,\"cus_bad\":%d,\"xcd\":%d,"
         "\"se\":%d,\"sh\":%d,\"cu\":%d,\"simd\":%d,\"fail_mask\":%u,\"first_fail_mask\":%u,"
         "\"n_bad\":%u,\"first_bad\":%u,\"bits_bad\":%u,\"first_bad_index\":%lld,",
         a.cus_seen, a.xcds_seen, a.simds_seen, a.cus_bad, a.xcd, a.se, a.sh, a.cu, a.simd,
         a.fail_mask, a.first_fail_mask, a.n_bad, a.first_bad, a.bits_bad, a.first_bad_index);
  printf("\"first_bad_round\":%d,\"first_bad_record\":%d,\"grid_blocks\":%d,\"iters\":%d,"
         "\"gpu_ms\":%.3f,\"t_total_ms\":%.3f,\"failed_test\":\"%s\",\"msg\":\"%s\"}",
         r.first_bad_round, r.first_bad_record, r.grid_blocks, r.iters, r.gpu_ms, r.t_total_ms,
         r.failed_test, r.msg);
}

// The ALU stage's result, keys as nodeops/alu.py run_alu.
void print_alu(const CroAluResult& r) {
  const CroAluAgg& a = r.agg;
  printf("\"alu\":{\"ok\":%s,\"rc\":%d,\"cus_expected\":%d,\"rounds\":%d,"
         "\"waves_run\":%llu,\"waves_bad\":%llu,",
         r.ok ? "true" : "false", r.rc, r.cus_expected, r.rounds, a.waves_run, a.waves_bad);
  for (int t = 0; t < CRO_ALU_TESTS; ++t) printf("\"bad_%s\":%llu,", kCroAluTestNames[t], a.bad[t]);
  printf("\"cus_seen\":%d,\"xcds_seen\":%d,\"simds_seen\":%d,\"cus_bad\":%d,\"xcd\":%d,"
         "\"se\":%d,\"sh\":%d,\"cu\":%d,\"simd\":%d,\"fail_mask\":%u,\"first_fail_mask\":%u,"
         "\"n_bad\":%u,\"first_bad\":%u,\"bits_bad\":%u,\"first_bad_index\":%lld,"
         "\"digest\":%u,\"no_majority\":%u,\"digest_waves\":%llu,",
         a.cus_seen, a.xcds_seen, a.simds_seen, a.cus_bad, a.xcd, a.se, a.sh, a.cu, a.simd,
         a.fail_mask, a.first_fail_mask, a.n_bad, a.first_bad, a.bits_bad, a.first_bad_index,
         a.digest, a.no_majority, a.digest_waves);
  printf("\"first_bad_round\":%d,\"first_bad_record\":%d,\"grid_blocks\":%d,\"iters\":%d,"
         "\"gpu_ms\":%.3f,\"t_total_ms\":%.3f,\"failed_test\":\"%s\",\"msg\":\"%s\"}",
         r.first_bad_round, r.first_bad_record, r.grid_blocks, r.iters, r.gpu_ms, r.t_total_ms,
         r.failed_test, r.msg);
}

int scrub_unavailable(const std::string& msg);
void* load_entry(const char* soname, const char* symbol, std::string* why);

// The quick probe first, then with --compute the compute-coverage stage, then
// with --formats the matrix-format stage, then with --coherence the coherence
// stage, then with --movement the data-movement stage, then with --alu the
// ALU stage, then with --deep the data-integrity stage; a device that failed a
// stage is not stressed further.  Top-level "ok" and "msg" cover all stages
// run.  The formats and coherence libraries are looked up before anything runs: a probe that was asked for the stage and cannot run it says
// so, in the scrubs' shape, and probes nothing.
int cmd_probe_staged(int device, bool compute, const CroComputeOpts& copts, bool deep,
                     const CroIntegrityOpts& opts, const CroFormatsOpts* fopts = nullptr,
                     const CroCoherenceOpts* hopts = nullptr,
                     const CroMovementOpts* mopts = nullptr,
                     const CroAluOpts* aopts = nullptr) {
  typedef int (*FormatsRun)(int, const CroFormatsOpts*, CroFormatsResult*);
  FormatsRun run_formats = nullptr;
  if (fopts) {
    std::string why;
    run_formats = (FormatsRun)load_entry("libcroformats.so", "cro_formats_run", &why);
    if (run_formats == nullptr) return scrub_unavailable(why);
  }
  typedef int (*CoherenceRun)(int, const CroCoherenceOpts*, CroCoherenceResult*);
  CoherenceRun run_coherence = nullptr;
  if (hopts) {
    std::string why;
    run_coherence = (CoherenceRun)load_entry("libcrocoherence.so", "cro_coherence_run", &why);
    if (run_coherence == nullptr) return scrub_unavailable(why);
  }
  typedef int (*MovementRun)(int, const CroMovementOpts*, CroMovementResult*);
  MovementRun run_movement = nullptr;
  if (mopts) {
    std::string why;
    run_movement = (MovementRun)load_entry("libcromovement.so", "cro_movement_run", &why);
    if (run_movement == nullptr) return scrub_unavailable(why);
  }
  typedef int (*AluRun)(int, const CroAluOpts*, CroAluResult*);
  AluRun run_alu = nullptr;
  if (aopts) {
    std::string why;
    run_alu = (AluRun)load_entry("libcroalu.so", "cro_alu_run", &why);
    if (run_alu == nullptr) return scrub_unavailable(why);
  }
  CroProbeResult result;
  int rc = cro_probe_run(device, &result);
  CroComputeResult comp;
  CroFormatsResult fmts;
  CroCoherenceResult coh;
  CroMovementResult mov;
  CroAluResult alu;
  CroIntegrityResult integ;
  bool ran_comp = false, ran_fmts = false, ran_coh = false, ran_mov = false, ran_alu = false;
  bool ran = false;
  bool ok = result.ok;
  const char* msg = result.msg;
  if (ok && compute) {
    cro_probe_compute(device, &copts, &comp);
    ran_comp = true;
    if (!comp.ok) {
      ok = false;
      msg = comp.msg;
    }
  }
  if (ok && run_formats) {
    run_formats(device, fopts, &fmts);
    ran_fmts = true;
    if (!fmts.ok) {
      ok = false;
      msg = fmts.msg;
    }
  }
  if (ok && run_coherence) {
    run_coherence(device, hopts, &coh);
    ran_coh = true;
    if (!coh.ok) {
      ok = false;
      msg = coh.msg;
    }
  }
  if (ok && run_movement) {
    run_movement(device, mopts, &mov);
    ran_mov = true;
    if (!mov.ok) {
      ok = false;
      msg = mov.msg;
    }
  }
  if (ok && run_alu) {
    run_alu(device, aopts, &alu);
    ran_alu = true;
    if (!alu.ok) {
      ok = false;
      msg = alu.msg;
    }
  }
  if (ok && deep) {
    cro_probe_integrity(device, &opts, &integ);
    ran = true;
    if (!integ.ok) {
      ok = false;
      msg = integ.msg;
    }
  }
  printf("{\"ok\":%s,\"rc\":%d,\"mfma_f32_exact\":%s,\"hbm_gbps\":%.1f,"
         "\"bf16_tflops\":%.1f,\"vram_total\":%lld,\"vram_free\":%lld,"
         "\"gcn_arch\":\"%s\",\"msg\":\"%s\"",
         ok ? "true" : "false", rc, result.mfma_f32_exact ? "true" : "false",
         result.hbm_gbps, result.bf16_tflops, result.vram_total, result.vram_free,
         result.gcn_arch, msg);
  if (ran_comp) {
    printf(",");
    print_compute(comp);
  }
  if (ran_fmts) {
    printf(",");
    print_formats(fmts);
  }
  if (ran_coh) {
    printf(",");
    print_coherence(coh);
  }
  if (ran_mov) {
    printf(",");
    print_movement(mov);
  }
  if (ran_alu) {
    printf(",");
    print_alu(alu);
  }
  if (ran) {
    printf(",");
    print_integrity(integ);
  }
  printf("}\n");
  return ok ? 0 : 1;
}

// `text` as the inside of a JSON string.
std::string json_escape(const char* text) {
  std::string out;
  for (const char* p = text; *p; ++p) {
    const unsigned char c = (unsigned char)*p;
    if (c == '"' || c == '\\') {
      out += '\\';
      out += (char)c;
    } else if (c < 0x20) {
      out += ' ';
    } else {
      out += (char)c;
    }
  }
  return out;
}

// A scrub that could not start: the same object with only these keys.
int scrub_unavailable(const std::string& msg) {
  printf("{\"ok\":false,\"rc\":-1,\"msg\":\"%s\"}\n", json_escape(msg.c_str()).c_str());
  return 1;
}

// The LDS scrub's result as one JSON object, keys as nodeops/ldsscrub.py
// run_lds_scrub.
void print_lds_scrub(const CroLdsScrubResult& r) {
  printf("{\"ok\":%s,\"rc\":%d,\"cus_expected\":%d,\"cus_seen\":%d,\"xcds_seen\":%d,"
         "\"rounds\":%d,\"lds_bytes\":%d,\"grid\":%d,\"workgroups\":%llu,"
         "\"bytes_scrubbed\":%llu,\"dirty_words_before\":%llu,\"dirty_workgroups\":%llu,",
         r.ok && r.rc == 0 ? "true" : "false", r.rc, r.cus_expected, r.cus_seen, r.xcds_seen,
         r.rounds, r.lds_bytes, r.grid, r.workgroups, r.bytes_scrubbed, r.dirty_words_before,
         r.dirty_workgroups);
  printf("\"n_bad\":%llu,\"guard_bad\":%llu,\"recheck_dirty_words\":%llu,"
         "\"first_dirty_word\":%u,\"first_bad_word\":%u,\"bits_bad\":%u,"
         "\"bad_workgroups\":%d,\"xcd\":%d,\"se\":%d,\"sh\":%d,\"cu\":%d,"
         "\"gpu_ms\":%.3f,\"t_total_ms\":%.1f,\"msg\":\"%s\"}",
         r.n_bad, r.guard_bad, r.recheck_dirty_words, r.first_dirty_word, r.first_bad_word,
         r.bits_bad, r.bad_workgroups, r.xcd, r.se, r.sh, r.cu, r.gpu_ms, r.t_total_ms,
         json_escape(r.msg).c_str());
}

// The register scrub's result as one JSON object, keys as nodeops/regscrub.py
// run_reg_scrub.
void print_reg_scrub(const CroRegScrubResult& r) {
  printf("{\"ok\":%s,\"rc\":%d,\"simds_expected\":%d,\"simds_seen\":%d,\"cus_seen\":%d,"
         "\"xcds_seen\":%d,\"rounds\":%d,\"grid\":%d,\"first_vgpr\":%d,"
         "\"regs_per_lane\":%d,\"waves\":%llu,\"bytes_scrubbed\":%llu,"
         "\"dirty_words_before\":%llu,\"dirty_waves\":%llu,",
         r.ok && r.rc == 0 ? "true" : "false", r.rc, r.simds_expected, r.simds_seen, r.cus_seen,
         r.xcds_seen, r.rounds, r.grid, r.first_vgpr, r.regs_per_lane, r.waves,
         r.bytes_scrubbed, r.dirty_words_before, r.dirty_waves);
  printf("\"n_bad\":%llu,\"recheck_dirty_words\":%llu,\"first_dirty_word\":%u,"
         "\"first_bad_word\":%u,\"bits_bad\":%u,\"bad_waves\":%d,\"xcd\":%d,\"se\":%d,"
         "\"sh\":%d,\"cu\":%d,\"simd\":%d,\"wave\":%d,\"gpu_ms\":%.3f,"
         "\"t_total_ms\":%.1f,\"msg\":\"%s\"}",
         r.n_bad, r.recheck_dirty_words, r.first_dirty_word, r.first_bad_word, r.bits_bad,
         r.bad_waves, r.xcd, r.se, r.sh, r.cu, r.simd, r.wave, r.gpu_ms, r.t_total_ms,
         json_escape(r.msg).c_str());
}

// The result as one JSON object, keys as nodeops/scrub.py run_scrub.  The LDS
// scrub's result is nested under "lds" and the register scrub's under "regs"
// after it, merged as nodeops/scrub.py merge_lds_result and merge_regs_result
// do: ok only if every stage passed; rc and msg are those of the first stage
// that failed, else the last stage's.  Returns the merged ok.
bool print_scrub(const CroScrubResult& r, const CroLdsScrubResult* lds,
                 const CroRegScrubResult* regs) {
  const bool vram_ok = r.ok && r.rc == 0;
  const bool lds_ok = lds == nullptr || (lds->ok && lds->rc == 0);
  const bool ok = vram_ok && lds_ok && (regs == nullptr || (regs->ok && regs->rc == 0));
  int rc = r.rc;
  const char* msg = r.msg;
  if (vram_ok && lds) {
    rc = lds->rc;
    msg = lds->msg;
  }
  if (vram_ok && lds_ok && regs) {
    rc = regs->rc;
    msg = regs->msg;
  }
  printf("{\"ok\":%s,\"rc\":%d,\"vram_total\":%lld,\"vram_free_before\":%lld,"
         "\"bytes_target\":%lld,\"bytes_scrubbed\":%lld,\"bytes_verified\":%lld,"
         "\"chunks\":%d,\"alloc_refusals\":%d,\"dirty_words_before\":%llu,",
         ok ? "true" : "false", rc, r.vram_total, r.vram_free_before,
         r.bytes_target, r.bytes_scrubbed, r.bytes_verified, r.chunks, r.alloc_refusals,
         r.dirty_words_before);
  printf("\"n_bad\":%llu,\"first_bad_byte\":%llu,\"bits_bad\":%u,\"first_bad_got\":%u,"
         "\"fraction\":%.6f,\"fill_gbps\":%.1f,\"verify_gbps\":%.1f,\"census_gbps\":%.1f,"
         "\"t_alloc_ms\":%.1f,\"t_total_ms\":%.1f,\"msg\":\"%s\"",
         r.n_bad, r.first_bad_byte, r.bits_bad, r.first_bad_got, r.fraction, r.fill_gbps,
         r.verify_gbps, r.census_gbps, r.t_alloc_ms, r.t_total_ms, json_escape(msg).c_str());
  if (lds) {
    printf(",\"lds\":");
    print_lds_scrub(*lds);
  }
  if (regs) {
    printf(",\"regs\":");
    print_reg_scrub(*regs);
  }
  printf("}\n");
  return ok;
}

// `symbol` of `soname`, loaded here and not linked, so an agent on a node
// without the library still serves every other subcommand; the agent's
// RUNPATH finds it next to libcroprobe.so.  Null with the reason in *why.
void* load_entry(const char* soname, const char* symbol, std::string* why) {
  void* lib = dlopen(soname, RTLD_NOW | RTLD_LOCAL);
  if (lib == nullptr) {
    const char* err = dlerror();
    *why = std::string(soname) + " not available: " + (err ? err : "");
    return nullptr;
  }
  void* entry = dlsym(lib, symbol);
  if (entry == nullptr) *why = std::string(soname) + " not available: no symbol " + symbol;
  return entry;
}

// Every library is looked up before anything runs: a scrub that was asked to
// cover LDS or the registers and cannot says so and scrubs nothing.
int cmd_scrub(int device, const CroScrubOpts& opts, const CroLdsScrubOpts* lds_opts,
              const CroRegScrubOpts* reg_opts) {
  typedef int (*ScrubRun)(int, const CroScrubOpts*, CroScrubResult*);
  typedef int (*LdsScrubRun)(int, const CroLdsScrubOpts*, CroLdsScrubResult*);
  typedef int (*RegScrubRun)(int, const CroRegScrubOpts*, CroRegScrubResult*);
  std::string why;
  const ScrubRun run = (ScrubRun)load_entry("libcroscrub.so", "cro_scrub_run", &why);
  if (run == nullptr) return scrub_unavailable(why);
  LdsScrubRun run_lds = nullptr;
  if (lds_opts) {
    run_lds = (LdsScrubRun)load_entry("libcroldsscrub.so", "cro_lds_scrub_run", &why);
    if (run_lds == nullptr) return scrub_unavailable(why);
  }
  RegScrubRun run_regs = nullptr;
  if (reg_opts) {
    run_regs = (RegScrubRun)load_entry("libcroregscrub.so", "cro_reg_scrub_run", &why);
    if (run_regs == nullptr) return scrub_unavailable(why);
  }
  CroScrubResult result;
  run(device, &opts, &result);
  CroLdsScrubResult lds_result;
  if (run_lds) run_lds(device, lds_opts, &lds_result);
  CroRegScrubResult reg_result;
  if (run_regs) run_regs(device, reg_opts, &reg_result);
  return print_scrub(result, run_lds ? &lds_result : nullptr,
                     run_regs ? &reg_result : nullptr) ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: croagent <list|cxl|pids|probe|scrub|drain|rescan> [options]\n");
    return 2;
  }
  std::string cmd = argv[1];
  std::string bdf;
  long long gpu_id = -1;
  int device = 0;
  bool deep = false, compute = false;
  CroIntegrityOpts integ_opts;
  memset(&integ_opts, 0, sizeof(integ_opts));
  CroComputeOpts compute_opts;  // no self-test options here: those are for tests
  memset(&compute_opts, 0, sizeof(compute_opts));
  CroScrubOpts scrub_opts;  // no self-test options here either
  memset(&scrub_opts, 0, sizeof(scrub_opts));
  bool lds = false;
  CroLdsScrubOpts lds_opts;  // nor here
  memset(&lds_opts, 0, sizeof(lds_opts));
  bool regs = false;
  CroRegScrubOpts reg_opts;  // nor here
  memset(&reg_opts, 0, sizeof(reg_opts));
  bool formats = false;
  CroFormatsOpts formats_opts;  // nor here
  memset(&formats_opts, 0, sizeof(formats_opts));
  bool coherence = false;
  CroCoherenceOpts coherence_opts;  // nor here
  memset(&coherence_opts, 0, sizeof(coherence_opts));
  bool movement = false;
  CroMovementOpts movement_opts;  // nor here
  memset(&movement_opts, 0, sizeof(movement_opts));
  bool alu = false;
  CroAluOpts alu_opts;  // nor here
  memset(&alu_opts, 0, sizeof(alu_opts));
  for (int i = 2; i < argc; ++i) {
    std::string arg = argv[i];
    if (arg == "--sysroot" && i + 1 < argc) g_sysroot = argv[++i];
    else if (arg == "--bdf" && i + 1 < argc) bdf = argv[++i];
    else if (arg == "--gpu-id" && i + 1 < argc) gpu_id = atoll(argv[++i]);
    else if (arg == "--device" && i + 1 < argc) device = atoi(argv[++i]);
    else if (arg == "--deep") deep = true;
    else if (arg == "--compute") compute = true;
    else if (arg == "--compute-min-cu-fraction" && i + 1 < argc) compute_opts.min_cu_fraction = atof(argv[++i]);
    else if (arg == "--formats") formats = true;
    else if (arg == "--formats-min-cu-fraction" && i + 1 < argc) formats_opts.min_cu_fraction = atof(argv[++i]);
    else if (arg == "--coherence") coherence = true;
    else if (arg == "--coherence-min-cu-fraction" && i + 1 < argc) coherence_opts.min_cu_fraction = atof(argv[++i]);
    else if (arg == "--movement") movement = true;
    else if (arg == "--movement-min-cu-fraction" && i + 1 < argc) movement_opts.min_cu_fraction = atof(argv[++i]);
    else if (arg == "--alu") alu = true;
    else if (arg == "--alu-min-cu-fraction" && i + 1 < argc) alu_opts.min_cu_fraction = atof(argv[++i]);
    else if (arg == "--vram-mib" && i + 1 < argc) integ_opts.vram_bytes = atoll(argv[++i]) << 20;
    else if (arg == "--link-mib" && i + 1 < argc) integ_opts.link_bytes = atoll(argv[++i]) << 20;
    else if (arg == "--link-floor-gbps" && i + 1 < argc) integ_opts.link_floor_gbps = atof(argv[++i]);
    else if (arg == "--max-mib" && i + 1 < argc) scrub_opts.max_bytes = atoll(argv[++i]) << 20;
    else if (arg == "--reserve-mib" && i + 1 < argc) scrub_opts.reserve_bytes = atoll(argv[++i]) << 20;
    else if (arg == "--min-fraction" && i + 1 < argc) scrub_opts.min_fraction = atof(argv[++i]);
    else if (arg == "--lds") lds = true;
    else if (arg == "--lds-min-cu-fraction" && i + 1 < argc) lds_opts.min_cu_fraction = atof(argv[++i]);
    else if (arg == "--regs") regs = true;
    else if (arg == "--regs-min-simd-fraction" && i + 1 < argc) reg_opts.min_simd_fraction = atof(argv[++i]);
  }
  if (cmd == "list") return cmd_list();
  if (cmd == "cxl") return cmd_cxl();
  if (cmd == "pids") return cmd_pids(gpu_id);
  if (cmd == "probe") {
    if (!bdf.empty()) {
      std::string lower = bdf;
      for (auto& c : lower) c = tolower(c);
      device = resolve_device_by_bdf(lower);
      if (device < 0) {
        fprintf(stderr, "no HIP device with bdf %s\n", bdf.c_str());
        return 1;
      }
    }
    return cmd_probe_staged(device, compute, compute_opts, deep, integ_opts,
                            formats ? &formats_opts : nullptr,
                            coherence ? &coherence_opts : nullptr,
                            movement ? &movement_opts : nullptr, alu ? &alu_opts : nullptr);
  }
  if (cmd == "scrub") {
    if (!bdf.empty()) {
      std::string lower = bdf;
      for (auto& c : lower) c = tolower(c);
      device = resolve_device_by_bdf(lower);
      if (device < 0) return scrub_unavailable("no HIP device with bdf " + bdf);
    }
    return cmd_scrub(device, scrub_opts, lds ? &lds_opts : nullptr, regs ? &reg_opts : nullptr);
  }
  if (cmd == "drain") return cmd_drain(bdf);
  if (cmd == "rescan") return cmd_rescan();
  fprintf(stderr, "unknown command %s\n", cmd.c_str());
  return 2;
}
