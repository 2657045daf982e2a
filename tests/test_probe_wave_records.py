"""CPU test of what the per-wave probe stages (compute coverage, matrix
formats, data movement) share on the host: one aggregation over one record
layout.  A small host program (host C++ compiler, no HIP, no GPU) feeds the
same record bytes to cro_coverage_aggregate, cro_formats_aggregate and
cro_movement_aggregate and to the core they are built on; the three must
agree wherever they hold the same thing, and each must equal its numpy
mirror."""

import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from cro_amd.nodeops import formats as F
from cro_amd.nodeops import movement as M
from cro_amd.nodeops import probe as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(REPO, "cro_amd", "hip")
FIELDS = ("xcc_id", "hw_id", "fail_mask", "n_bad", "first_bad", "bits_bad", "valid", "reserved")

WAVE_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "croprobe.h"
#include "croformats.h"
#include "cromovement.h"

#define COMMON_FMT "\"waves_run\":%llu,\"waves_bad\":%llu,\"first_bad_index\":%lld,"          \
  "\"cus_seen\":%d,\"xcds_seen\":%d,\"simds_seen\":%d,\"cus_bad\":%d,\"xcd\":%d,\"se\":%d,"  \
  "\"sh\":%d,\"cu\":%d,\"simd\":%d,\"first_fail_mask\":%u,\"n_bad\":%u,\"first_bad\":%u,"     \
  "\"bits_bad\":%u"
#define COMMON(a) (a).waves_run, (a).waves_bad, (a).first_bad_index, (a).cus_seen,           \
  (a).xcds_seen, (a).simds_seen, (a).cus_bad, (a).xcd, (a).se, (a).sh, (a).cu, (a).simd,     \
  (a).first_fail_mask, (a).n_bad, (a).first_bad, (a).bits_bad

static void list(const char* name, const unsigned long long* v, int n) {
  printf(",\"%s\":[", name);
  for (int i = 0; i < n; ++i) printf("%s%llu", i ? "," : "", v[i]);
  printf("]");
}

static void keys(const unsigned int* v, int n) {
  printf(",\"n_bad_cu_keys\":%d,\"bad_cu_keys\":[", n);
  for (int i = 0; i < n; ++i) printf("%s%u", i ? "," : "", v[i]);
  printf("]");
}

int main() {
  std::vector<CroCoverageRecord> cov;
  CroCoverageRecord r;
  while (scanf("%u %u %u %u %u %u %u %u", &r.xcc_id, &r.hw_id, &r.fail_mask, &r.n_bad,
               &r.first_bad, &r.bits_bad, &r.valid, &r.reserved) == 8)
    cov.push_back(r);
  // the same bytes under each stage's record type
  const size_t n = cov.size(), bytes = n * sizeof(CroCoverageRecord);
  std::vector<CroFormatsRecord> fmt(n);
  std::vector<CroMovementRecord> mov(n);
  memcpy(fmt.data(), cov.data(), bytes);
  memcpy(mov.data(), cov.data(), bytes);

  CroWaveSummary s;
  CroCoverageAgg c;
  CroFormatsAgg f;
  CroMovementAgg m;
  cro_wave_summarize(cov.data(), n, &s);
  cro_coverage_aggregate(cov.data(), n, 256, &c);
  cro_formats_aggregate(fmt.data(), n, &f);
  cro_movement_aggregate(mov.data(), n, &m);

  printf("{\"summary\":{" COMMON_FMT ",\"fail_mask\":%u", COMMON(s), s.fail_mask);
  list("bad", s.bad, CRO_COV_MAX_MASK_BITS);
  keys(s.bad_cu_keys, s.n_bad_cu_keys);
  printf("},\"compute\":{" COMMON_FMT, COMMON(c));
  const unsigned long long cbad[CRO_COV_TESTS] = {c.bad_f32, c.bad_i8, c.bad_bf16, c.bad_lds};
  list("bad", cbad, CRO_COV_TESTS);
  keys(c.bad_cu_keys, c.n_bad_cu_keys);
  printf("},\"formats\":{" COMMON_FMT, COMMON(f));
  list("bad", f.bad, CRO_FMT_TESTS);
  printf("},\"movement\":{" COMMON_FMT ",\"fail_mask\":%u", COMMON(m), m.fail_mask);
  list("bad", m.bad, CRO_MOV_TESTS);
  printf("}}\n");
  return 0;
}
"""

COMMON = ("waves_run", "waves_bad", "first_bad_index", "cus_seen", "xcds_seen", "simds_seen",
          "cus_bad", "xcd", "se", "sh", "cu", "simd", "first_fail_mask", "n_bad", "first_bad",
          "bits_bad")


def _host_cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    pytest.fail("no host C++ compiler (c++/g++/clang++) on PATH")


def _hw(se, sh, cu, simd, slot=0):
    return (se << 13) | (sh << 12) | (cu << 8) | (simd << 4) | slot


def wave_rows():
    """300 records, two rounds of 150: record i of a round is wave i % 4 of
    workgroup i // 4, the workgroups on 38 CUs of 4 XCDs, in the second round
    shifted by one SIMD.  Five records were never written (one of them holds a
    fail mask all the same), nine CUs have a bad wave (one of them twice, one in
    both rounds), the masks have one to five bits set up to bit 9, and the
    first bad record is record 21."""
    bad = {21: 0b0000101000, 22: 0b1000000001, 40: 0b0001000110, 41: 0b0000101000,
           57: 0b0000010000, 76: 0b1111100000, 95: 0b0000000110, 118: 0b0100000001,
           133: 0b0000001111, 149: 0b0010000000,
           150 + 21: 0b0000000001, 150 + 64: 0b1010101010}
    unwritten = {0, 7, 22, 150, 299}
    rows = []
    for i in range(300):
        rnd, rec = divmod(i, 150)
        group, wave = divmod(rec, 4)
        xcd, se, sh, cu = group % 4, (group // 4) % 5, group % 2, (group // 8) % 16
        mask = bad.get(i, 0)
        rows.append((
            xcd | 0xABC0,  # only bits 3:0 are the XCD
            _hw(se, sh, cu, (wave + rnd) % 4, slot=i % 10),
            mask,
            bin(mask).count("1") * 3 if mask else 0,
            (i * 2654435761) & 0xFFFFFFFF if mask else 0xFFFFFFFF,
            (0x80000001 << (i % 5)) & 0xFFFFFFFF if mask else 0,
            0 if i in unwritten else 1 + i % 3,  # any non-zero value is "written"
            0,
        ))
    for i in unwritten:  # whatever an unwritten record holds is ignored
        rows[i] = rows[i][:2] + (0b11, 5, 5, 5, 0, 0)
    return rows


@pytest.fixture(scope="module")
def wave_results(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wave-records")
    src = tmp / "wave_main.cpp"
    src.write_text(WAVE_MAIN)
    exe = tmp / "wave_main"
    subprocess.run([_host_cxx(), "-std=c++17", "-O1", f"-I{HIP_DIR}", str(src), "-o",
                    str(exe)], check=True, capture_output=True, text=True)
    rows = wave_rows()
    text = "\n".join(" ".join(str(x) for x in r) for r in rows) + "\n"
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    dtype = np.dtype([(name, np.uint32) for name in FIELDS])
    return np.array(rows, dtype=dtype), json.loads(run.stdout)


def test_three_stage_aggregates_agree_with_each_other_and_with_the_one_mirror(wave_results):
    rec, got = wave_results
    s, c, f, m = (got[k] for k in ("summary", "compute", "formats", "movement"))

    # the input is what it claims to be
    assert rec.size == 300 and s["waves_run"] == 295
    assert s["cus_bad"] == 9 and s["n_bad_cu_keys"] == 8 and s["waves_bad"] == 11
    assert s["first_bad_index"] == 21 and s["first_fail_mask"] == 0b0000101000
    # (the last workgroup has two waves a round, and its last record is unwritten)
    assert s["cus_seen"] == 38 and s["xcds_seen"] == 4 and s["simds_seen"] == 4 * 37 + 2
    assert len(set(s["bad_cu_keys"])) == 8

    # the three stages agree wherever they hold the same thing
    for name in COMMON:
        assert s[name] == c[name] == f[name] == m[name], name
    assert c["bad"] == s["bad"][:4] and f["bad"] == s["bad"][:7] and m["bad"] == s["bad"][:10]
    assert s["bad"][10:] == [0] * 22
    assert (c["n_bad_cu_keys"], c["bad_cu_keys"]) == (s["n_bad_cu_keys"], s["bad_cu_keys"])
    assert m["fail_mask"] == s["fail_mask"] == 0b1111111111

    # and each equals the numpy mirror
    bits = tuple(str(b) for b in range(32))
    common, fail_mask, bad_keys = P.aggregate_wave_records(rec, bits)
    want = {k: common[k] for k in COMMON}
    want.update(bad=[common[f"bad_{b}"] for b in bits], fail_mask=fail_mask,
                n_bad_cu_keys=8, bad_cu_keys=bad_keys[:8])
    assert s == want and len(bad_keys) == 9

    def flat(agg, names):
        out = {k: v for k, v in agg.items() if k != "bad"}
        out.update({f"bad_{name}": n for name, n in zip(names, agg["bad"])})
        return out

    assert flat(c, ("f32", "i8", "bf16", "lds")) == P.aggregate_records(rec)
    assert flat(f, F.FORMATS_TESTS) == F.aggregate_formats_records(rec)
    assert flat(m, M.MOVEMENT_TESTS) == M.aggregate_movement_records(rec)
