"""CPU tests of the compute-coverage probe stage: record decode, aggregation
and the expected tiles of crocoverage.h against their numpy mirrors (through
a small host program built with the host C++ compiler — no HIP, no GPU), the
two C structs against their ctypes mirrors, the stage plumbing, the
controller's handling of a compute result, and the operator flags."""

import argparse
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from cro_amd.api.v1alpha1.types import ComposableResource, Event
from cro_amd.fabric.base import FabricError
from cro_amd.nodeops import probe as probe_mod
from tests.conftest import make_node, make_resource

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(REPO, "cro_amd", "hip")


def _host_cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    pytest.fail("no host C++ compiler (c++/g++/clang++) on PATH")


def _build(tmp_path, name, source):
    src = tmp_path / f"{name}.cpp"
    src.write_text(source)
    exe = tmp_path / name
    subprocess.run(
        [_host_cxx(), "-std=c++17", "-O1", "-ffp-contract=off", f"-I{HIP_DIR}", str(src),
         "-o", str(exe)],
        check=True, capture_output=True, text=True,
    )
    return str(exe)


# -- decode and aggregation ---------------------------------------------------------

COVERAGE_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "crocoverage.h"

static int tiles(unsigned seed) {
  static float A32[16 * 64], B32[64 * 16], E32[256];
  static int8_t A8[16 * 256], B8[256 * 16];
  static int32_t E8[256];
  static int Ai[32 * 64], Bi[64 * 32];
  static uint16_t A16[32 * 64], B16[64 * 32];
  static float E16[1024];
  cro_cov_make_f32(seed, A32, B32);
  cro_cov_ref_f32(A32, B32, E32);
  cro_cov_make_i8(seed, A8, B8);
  cro_cov_ref_i8(A8, B8, E8);
  cro_cov_make_bf16(seed, Ai, Bi, A16, B16);
  cro_cov_ref_bf16(Ai, Bi, E16);
  auto bits = [](float f) { unsigned u; memcpy(&u, &f, 4); return u; };
  printf("A32"); for (float v : A32) printf(" %u", bits(v)); printf("\n");
  printf("B32"); for (float v : B32) printf(" %u", bits(v)); printf("\n");
  printf("E32"); for (float v : E32) printf(" %u", bits(v)); printf("\n");
  printf("A8"); for (int8_t v : A8) printf(" %d", (int)v); printf("\n");
  printf("B8"); for (int8_t v : B8) printf(" %d", (int)v); printf("\n");
  printf("E8"); for (int32_t v : E8) printf(" %d", v); printf("\n");
  printf("A16"); for (int v : Ai) printf(" %d", v); printf("\n");
  printf("B16"); for (int v : Bi) printf(" %d", v); printf("\n");
  printf("A16bits"); for (uint16_t v : A16) printf(" %u", (unsigned)v); printf("\n");
  printf("B16bits"); for (uint16_t v : B16) printf(" %u", (unsigned)v); printf("\n");
  printf("E16"); for (float v : E16) printf(" %u", bits(v)); printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "tiles")) return tiles((unsigned)strtoul(argv[2], nullptr, 10));
  if (argc == 2 && !strcmp(argv[1], "sizes")) {
    printf("%zu %zu\n", sizeof(CroCoverageRecord), sizeof(CroCoverageAgg));
    return 0;
  }
  // records on stdin, eight unsigned words each
  std::vector<CroCoverageRecord> recs;
  unsigned w[8];
  while (scanf("%u %u %u %u %u %u %u %u", w, w + 1, w + 2, w + 3, w + 4, w + 5, w + 6, w + 7) == 8) {
    CroCoverageRecord r = {w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
    recs.push_back(r);
  }
  for (const auto& r : recs) {
    CroCoverageLoc l = cro_cov_decode(r.xcc_id, r.hw_id);
    CroCoverageLoc k = cro_cov_decode_key(cro_cov_cu_key(r.xcc_id, r.hw_id));
    printf("loc %u %u %u %u %u %u key %u %u %u %u %u\n", l.xcd, l.se, l.sh, l.cu, l.simd,
           l.wave_slot, cro_cov_cu_key(r.xcc_id, r.hw_id), k.xcd, k.se, k.sh, k.cu);
  }
  CroCoverageAgg a;
  cro_coverage_aggregate(recs.data(), recs.size(), 256, &a);
  printf("waves_run %llu\nwaves_bad %llu\nbad_f32 %llu\nbad_i8 %llu\nbad_bf16 %llu\nbad_lds %llu\n",
         a.waves_run, a.waves_bad, a.bad_f32, a.bad_i8, a.bad_bf16, a.bad_lds);
  printf("first_bad_index %lld\ncus_seen %d\nxcds_seen %d\nsimds_seen %d\ncus_bad %d\n",
         a.first_bad_index, a.cus_seen, a.xcds_seen, a.simds_seen, a.cus_bad);
  printf("xcd %d\nse %d\nsh %d\ncu %d\nsimd %d\n", a.xcd, a.se, a.sh, a.cu, a.simd);
  printf("first_fail_mask %u\nn_bad %u\nfirst_bad %u\nbits_bad %u\nn_bad_cu_keys %d\n",
         a.first_fail_mask, a.n_bad, a.first_bad, a.bits_bad, a.n_bad_cu_keys);
  printf("bad_cu_keys");
  for (int i = 0; i < a.n_bad_cu_keys; ++i) printf(" %u", a.bad_cu_keys[i]);
  printf("\ntest_name %s.\n", cro_cov_test_name(a.first_fail_mask));
  return 0;
}
"""

RECORD_DTYPE = np.dtype([(name, np.uint32) for name, _ in probe_mod.CroCoverageRecord._fields_])
NONE32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def coverage_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("coverage"), "coverage_main", COVERAGE_MAIN)


def hw_id(se, sh, cu, simd, wave_slot=0, high=0):
    """A raw HW_ID word; ``high`` fills bits 31:16 (other fields) and the
    PIPE_ID bits 7:6, which the decode must ignore."""
    return (
        (high << 16) | (se << 13) | (sh << 12) | (cu << 8) | ((high & 3) << 6) | (simd << 4)
        | wave_slot
    )


def rec(xcd, se, cu, simd, mask=0, n_bad=0, first_bad=NONE32, bits=0, sh=0, valid=1, high=0x5A3):
    # XCC_ID carries other fields above bit 3: the decode keeps bits 3:0
    return (xcd | 0x30, hw_id(se, sh, cu, simd, wave_slot=simd + 1, high=high), mask, n_bad,
            first_bad, bits, valid, 0)


def _records(rows):
    return np.array(rows, dtype=RECORD_DTYPE)


def _run_aggregate(exe, records):
    text = "\n".join(" ".join(str(int(v)) for v in row) for row in records.tolist()) + "\n"
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout
    locs, agg = [], {}
    for line in out.splitlines():
        parts = line.split()
        if parts[0] == "loc":
            locs.append([int(v) for v in parts[1:7]] + [int(v) for v in parts[8:]])
        elif parts[0] == "bad_cu_keys":
            agg["bad_cu_keys"] = [int(v) for v in parts[1:]]
        elif parts[0] == "test_name":
            agg["test_name"] = line.split(" ", 1)[1][:-1]
        else:
            agg[parts[0]] = int(parts[1])
    return locs, agg


def _check_against_numpy(exe, records):
    locs, agg = _run_aggregate(exe, records)
    assert len(locs) == len(records)
    for row, got in zip(records, locs):
        loc = probe_mod.decode_location(int(row["xcc_id"]), int(row["hw_id"]))
        key = probe_mod.cu_key(int(row["xcc_id"]), int(row["hw_id"]))
        kloc = probe_mod.decode_cu_key(key)
        assert got == [loc["xcd"], loc["se"], loc["sh"], loc["cu"], loc["simd"],
                       loc["wave_slot"], key, kloc["xcd"], kloc["se"], kloc["sh"], kloc["cu"]]
    ref = probe_mod.aggregate_records(records)
    name = agg.pop("test_name")
    assert agg == ref
    return agg, name


def _full_chip(rounds=1):
    """8 XCDs x 4 SEs x 8 CUs x 4 SIMDs, one wave each per round."""
    rows = []
    for _ in range(rounds):
        for xcd in range(8):
            for se in range(4):
                for cu in range(8):
                    for simd in range(4):
                        rows.append(rec(xcd, se, cu, simd))
    return rows


def test_decode_fields():
    word = hw_id(se=5, sh=1, cu=11, simd=2, wave_slot=9, high=0xBEEF)
    assert probe_mod.decode_location(0x37, word) == {
        "xcd": 7, "se": 5, "sh": 1, "cu": 11, "simd": 2, "wave_slot": 9,
    }
    key = probe_mod.cu_key(0x37, word)
    assert key == (7 << 16) | (5 << 13) | (1 << 12) | (11 << 8)
    assert probe_mod.decode_cu_key(key) == {"xcd": 7, "se": 5, "sh": 1, "cu": 11}


def test_aggregate_clean_full_chip_with_duplicates_across_rounds(coverage_exe):
    agg, name = _check_against_numpy(coverage_exe, _records(_full_chip(rounds=2)))
    assert agg["waves_run"] == 2 * 1024 and agg["waves_bad"] == 0
    assert (agg["cus_seen"], agg["xcds_seen"], agg["simds_seen"]) == (256, 8, 1024)
    assert agg["cus_bad"] == 0 and agg["first_bad_index"] == -1 and agg["bad_cu_keys"] == []
    assert (agg["xcd"], agg["se"], agg["cu"], agg["simd"]) == (-1, -1, -1, -1)
    assert agg["first_bad"] == NONE32 and name == ""


def test_aggregate_cu_with_three_simds_and_unwritten_records(coverage_exe):
    rows = [rec(0, 0, 0, s) for s in range(4)] + [rec(0, 1, 0, s) for s in (0, 1, 3)]
    rows.append(rec(3, 2, 5, 1, valid=0))  # never written: counts for nothing
    rows.append(rec(0, 1, 0, 1, sh=1))  # SH is part of the CU key
    agg, _ = _check_against_numpy(coverage_exe, _records(rows))
    assert agg["waves_run"] == 8
    assert (agg["cus_seen"], agg["xcds_seen"], agg["simds_seen"]) == (3, 1, 8)


def test_aggregate_one_bad_wave(coverage_exe):
    rows = _full_chip()
    at = 777
    xcd, se, cu, simd = 6, 0, 2, 1
    assert rows[at][:2] == rec(xcd, se, cu, simd)[:2]
    rows[at] = rec(xcd, se, cu, simd, mask=4, n_bad=3, first_bad=1000, bits=0x00400001)
    agg, name = _check_against_numpy(coverage_exe, _records(rows))
    assert agg["waves_bad"] == 1 and agg["cus_bad"] == 1 and agg["first_bad_index"] == at
    assert (agg["xcd"], agg["se"], agg["sh"], agg["cu"], agg["simd"]) == (xcd, se, 0, cu, simd)
    assert (agg["n_bad"], agg["first_bad"], agg["bits_bad"]) == (3, 1000, 0x00400001)
    assert agg["bad_cu_keys"] == [probe_mod.cu_key(xcd, hw_id(se, 0, cu, 0))]
    assert (agg["bad_f32"], agg["bad_i8"], agg["bad_bf16"], agg["bad_lds"]) == (0, 0, 1, 0)
    assert name == "mfma_bf16"


def test_aggregate_nine_bad_cus_caps_keys_at_eight(coverage_exe):
    rows = _full_chip(rounds=2)
    # nine CUs, given out of order; one of them bad on two SIMDs and in both rounds
    bad_at = [1500, 40, 41, 900, 100, 200, 300, 400, 500, 600, 1024 + 40]
    for i in bad_at:
        xcc, hw = rows[i][:2]
        rows[i] = (xcc, hw, 1, 1, 17, 0x80, 1, 0)
    records = _records(rows)
    agg, name = _check_against_numpy(coverage_exe, records)
    keys = []
    for i in sorted(bad_at):
        key = probe_mod.cu_key(int(records["xcc_id"][i]), int(records["hw_id"][i]))
        if key not in keys:
            keys.append(key)
    assert len(keys) == 9
    assert agg["waves_bad"] == len(bad_at) and agg["cus_bad"] == 9
    assert agg["n_bad_cu_keys"] == 8 and agg["bad_cu_keys"] == keys[:8]
    assert agg["first_bad_index"] == 40 and name == "mfma_f32"


def test_aggregate_first_bad_is_lowest_round_then_record(coverage_exe):
    per_round = 1024
    rows = _full_chip(rounds=3)
    late_round_low_record = 2 * per_round + 3
    early_round_high_record = 1 * per_round + 900
    for i, mask, elem in ((late_round_low_record, 2, 5), (early_round_high_record, 8, 4097)):
        xcc, hw = rows[i][:2]
        rows[i] = (xcc, hw, mask, 2, elem, 0x10, 1, 0)
    agg, name = _check_against_numpy(coverage_exe, _records(rows))
    assert agg["first_bad_index"] == early_round_high_record
    assert agg["first_bad"] == 4097 and name == "lds"
    assert agg["first_bad_index"] // per_round == 1 and agg["first_bad_index"] % per_round == 900


def test_aggregate_per_test_counts_from_fail_mask(coverage_exe):
    rows = _full_chip()
    masks = [1, 2, 4, 8, 3, 12, 15, 6, 9, 1, 8]
    for i, mask in enumerate(masks):
        xcc, hw = rows[10 * i + 2][:2]
        rows[10 * i + 2] = (xcc, hw, mask, 1, 0, 1, 1, 0)
    agg, name = _check_against_numpy(coverage_exe, _records(rows))
    assert agg["waves_bad"] == len(masks)
    assert agg["bad_f32"] == sum(1 for m in masks if m & 1) == 5
    assert agg["bad_i8"] == sum(1 for m in masks if m & 2) == 4
    assert agg["bad_bf16"] == sum(1 for m in masks if m & 4) == 4
    assert agg["bad_lds"] == sum(1 for m in masks if m & 8) == 5
    assert name == "mfma_f32"


def test_test_name_is_lowest_mask_bit(coverage_exe):
    for mask, want in ((2, "mfma_i8"), (12, "mfma_bf16"), (8, "lds"), (10, "mfma_i8")):
        _, agg = _run_aggregate(coverage_exe, _records([rec(0, 0, 0, 0, mask=mask, n_bad=1)]))
        assert agg["test_name"] == want
        assert probe_mod.COMPUTE_TESTS[(mask & -mask).bit_length() - 1] == want


# -- expected tiles -------------------------------------------------------------------


def _tiles_from_header(exe, seed):
    out = subprocess.run([exe, "tiles", str(seed)], check=True, capture_output=True,
                         text=True).stdout
    return {line.split()[0]: [int(v) for v in line.split()[1:]] for line in out.splitlines()}


@pytest.mark.parametrize("seed", [0, 0x1234ABCD])
def test_inputs_and_expected_tiles_match_header(coverage_exe, seed):
    hdr = _tiles_from_header(coverage_exe, seed)
    inputs = probe_mod.compute_inputs(seed)
    tiles = probe_mod.compute_expected_tiles(seed)

    def f32_bits(a):
        return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).ravel().tolist()

    assert f32_bits(inputs["f32"][0]) == hdr["A32"]
    assert f32_bits(inputs["f32"][1]) == hdr["B32"]
    assert f32_bits(tiles["f32"]) == hdr["E32"]  # bit-exact fmaf chain
    assert inputs["i8"][0].ravel().tolist() == hdr["A8"]
    assert inputs["i8"][1].ravel().tolist() == hdr["B8"]
    assert tiles["i8"].ravel().tolist() == hdr["E8"]
    assert inputs["bf16"][0].ravel().tolist() == hdr["A16"]
    assert inputs["bf16"][1].ravel().tolist() == hdr["B16"]
    assert probe_mod.bf16_bits(inputs["bf16"][0]).ravel().tolist() == hdr["A16bits"]
    assert probe_mod.bf16_bits(inputs["bf16"][1]).ravel().tolist() == hdr["B16bits"]
    assert f32_bits(tiles["bf16"]) == hdr["E16"]


def test_f32_inputs_are_the_quick_probes():
    """Seed 0: the LCG chain of cro_probe_run (probe.hip), A then B."""
    s, vals = 0x9E3779B9, []
    for _ in range(2 * 16 * 64):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        vals.append(np.float32(s >> 8) / np.float32(16777216.0) - np.float32(0.5))
    a, b = probe_mod.compute_inputs(0)["f32"]
    assert np.array_equal(np.concatenate([a.ravel(), b.ravel()]), np.array(vals, np.float32))


def test_quick_probes_documented_inputs_are_the_headers_at_seed_0():
    """The quick probe takes its inputs from cro_cov_make_f32(0): the inputs the
    benchmark documents for it are bit for bit what compute_inputs(0) mirrors
    (and test_inputs_and_expected_tiles_match_header ties that to the header)."""
    import bench

    a, b = bench._probe_inputs()
    a0, b0 = probe_mod.compute_inputs(0)["f32"]
    for got, want in ((a, a0), (b, b0)):
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("seed", [0, 7])
def test_expected_tiles_are_plain_integer_matmuls(seed):
    inputs = probe_mod.compute_inputs(seed)
    tiles = probe_mod.compute_expected_tiles(seed)
    a8, b8 = inputs["i8"]
    assert a8.dtype == np.int8 and a8.shape == (16, 256) and b8.shape == (256, 16)
    ref8 = np.array([[sum(int(a8[r, k]) * int(b8[k, c]) for k in range(256))
                      for c in range(16)] for r in range(16)])
    assert tiles["i8"].dtype == np.int32 and np.array_equal(tiles["i8"], ref8)
    assert np.abs(ref8).max() <= 256 * 128 * 128
    # the whole int8 range, both extremes in A and in B
    for m in (a8, b8):
        assert m.min() == -128 and m.max() == 127 and np.unique(m).size == 256
    a16, b16 = inputs["bf16"]
    assert a16.shape == (32, 64) and b16.shape == (64, 32)
    ref16 = np.array([[sum(int(a16[r, k]) * int(b16[k, c]) for k in range(64))
                       for c in range(32)] for r in range(32)])
    assert tiles["bf16"].dtype == np.float32
    assert np.array_equal(tiles["bf16"].astype(np.int64), ref16)
    # every partial sum, in any order, is an integer <= 64 * 64: exact in f32
    assert np.abs(a16).max() * np.abs(b16).max() <= 64 and 64 * 64 < 2 ** 24


@pytest.mark.parametrize("seed", [0, 7])
def test_bf16_inputs_small_nonzero_nonuniform_asymmetric(seed):
    a16, b16 = probe_mod.compute_inputs(seed)["bf16"]
    for m in (a16, b16):
        assert np.abs(m).max() <= 8 and np.abs(m).min() >= 1
        assert np.unique(m).size == 16  # every value of [-8, 8] but 0
        # bf16 holds each exactly
        assert np.array_equal(
            (probe_mod.bf16_bits(m).astype(np.uint32) << 16).view(np.float32).reshape(m.shape), m
        )
    # no square block equals its transpose: a swapped index changes the tile
    for block in (a16[:, :32], a16[:, 32:], b16[:32, :], b16[32:, :]):
        assert not np.array_equal(block, block.T)
    a8, b8 = probe_mod.compute_inputs(seed)["i8"]
    assert not np.array_equal(a8[:, :16], a8[:, :16].T)
    assert not np.array_equal(b8[:16, :], b8[:16, :].T)


# -- structs --------------------------------------------------------------------------

AGG_NAMES = {name for name, _ in probe_mod.COMPUTE_AGG_FIELDS}


def _struct_main():
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "croprobe.h"', "int main() {"]
    for cname, mirror in (
        ("CroComputeOpts", probe_mod.CroComputeOpts),
        ("CroComputeResult", probe_mod.CroComputeResult),
        ("CroCoverageRecord", probe_mod.CroCoverageRecord),
    ):
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for field, _ in mirror._fields_:
            path = f"agg.{field}" if cname == "CroComputeResult" and field in AGG_NAMES else field
            lines.append(
                f'  printf("{cname} {field} %zu %zu\\n", offsetof({cname}, {path}), '
                f"sizeof((({cname}*)0)->{path}));"
            )
    lines.append('  printf("CroCoverageAgg sizeof %zu\\n", sizeof(CroCoverageAgg));')
    lines += ["  return 0;", "}"]
    return "\n".join(lines)


def test_compute_struct_layout_matches_ctypes(tmp_path):
    """Every field the ctypes mirrors name exists in the headers at the same
    offset and size, and the totals agree (so the headers have no extra one)."""
    exe = _build(tmp_path, "struct_main", _struct_main())
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    mirrors = {
        "CroComputeOpts": probe_mod.CroComputeOpts,
        "CroComputeResult": probe_mod.CroComputeResult,
        "CroCoverageRecord": probe_mod.CroCoverageRecord,
    }
    seen = 0
    for line in out.splitlines():
        parts = line.split()
        if parts[0] == "CroCoverageAgg":
            agg_size = sum(ctypes.sizeof(t) for _, t in probe_mod.COMPUTE_AGG_FIELDS)
            assert agg_size == int(parts[2]), line
            continue
        mirror = mirrors[parts[0]]
        if parts[1] == "sizeof":
            assert ctypes.sizeof(mirror) == int(parts[2]), line
        else:
            desc = getattr(mirror, parts[1])
            assert (desc.offset, desc.size) == (int(parts[2]), int(parts[3])), line
        seen += 1
    assert seen == 3 + sum(len(m._fields_) for m in mirrors.values())
    for mirror in mirrors.values():  # no padding holes
        end = 0
        for field, _ in mirror._fields_:
            desc = getattr(mirror, field)
            assert desc.offset == end, (mirror.__name__, field)
            end = desc.offset + desc.size
        assert end == ctypes.sizeof(mirror)
    assert ctypes.sizeof(probe_mod.CroCoverageRecord) == RECORD_DTYPE.itemsize == 32


# -- make_probe_fn ----------------------------------------------------------------------


class Gpu:
    pci_bdf = "0000:05:00.0"


GOOD_QUICK = {"ok": True, "rc": 0, "mfma_f32_exact": True, "hbm_gbps": 4000.0, "msg": "ok"}
GOOD_COMPUTE = {
    "ok": True, "rc": 0, "cus_expected": 256, "cus_seen": 256, "xcds_seen": 8,
    "simds_seen": 1024, "rounds": 1, "waves_run": 1024, "waves_bad": 0, "cus_bad": 0,
    "failed_test": "", "gpu_ms": 1.234, "msg": "ok",
}
BAD_COMPUTE = {
    "ok": False, "rc": -30, "cus_expected": 256, "cus_seen": 256, "xcds_seen": 8,
    "simds_seen": 1024, "rounds": 1, "waves_run": 1024, "waves_bad": 4, "cus_bad": 1,
    "failed_test": "mfma_i8", "xcd": 5, "se": 2, "sh": 0, "cu": 7, "simd": 3,
    "first_bad": 200, "bits_bad": 0x00400000, "n_bad": 16, "bad_cu_keys": [0x54700],
    "msg": "compute mismatch in mfma_i8 at xcd=5 se=2 sh=0 cu=7 simd=3",
}
GOOD_INTEGRITY = {
    "ok": True, "rc": 0, "n_bad": 0, "failed_stage": "", "msg": "ok",
    "vram_passes": 2, "vram_bytes_verified": 2 << 30,
    "h2d_dma_bytes_verified": 256 << 20, "d2h_dma_bytes_verified": 256 << 20,
    "h2d_dma_gbps": 51.5, "d2h_dma_gbps": 49.0,
}
BAD_INTEGRITY = {
    "ok": False, "rc": -20, "n_bad": 3, "first_bad_byte": 4096, "bits_bad": 0x10,
    "failed_stage": "vram", "msg": "data mismatch in stage vram",
}


def _patch_probe(monkeypatch, quick, compute, integrity):
    order = []

    def run_probe(device=0):
        order.append(("quick", device, {}))
        return dict(quick)

    def run_compute(device=0, **kw):
        order.append(("compute", device, kw))
        return dict(compute)

    def run_integrity(device=0, **kw):
        order.append(("integrity", device, kw))
        return dict(integrity)

    monkeypatch.setattr(probe_mod, "hip_device_for_bdf", lambda bdf: 3)
    monkeypatch.setattr(probe_mod, "run_probe", run_probe)
    monkeypatch.setattr(probe_mod, "run_compute", run_compute)
    monkeypatch.setattr(probe_mod, "run_integrity", run_integrity)
    return order


def _stages(order):
    return [name for name, _, _ in order]


def test_compute_off_returns_todays_hooks(monkeypatch):
    assert probe_mod.make_probe_fn("quick") is probe_mod.probe_fn_for_nodeops
    assert probe_mod.make_probe_fn("quick", compute=False) is probe_mod.probe_fn_for_nodeops
    order = _patch_probe(monkeypatch, GOOD_QUICK, GOOD_COMPUTE, GOOD_INTEGRITY)
    deep = probe_mod.make_probe_fn("deep")
    result = deep(Gpu())
    assert deep.level == "deep" and _stages(order) == ["quick", "integrity"]
    assert result == dict(GOOD_QUICK, integrity=GOOD_INTEGRITY)  # no "compute" key
    with pytest.raises(ValueError):
        probe_mod.make_probe_fn("thorough", compute=True)


def test_quick_plus_compute_order_and_result(monkeypatch):
    order = _patch_probe(monkeypatch, GOOD_QUICK, GOOD_COMPUTE, GOOD_INTEGRITY)
    fn = probe_mod.make_probe_fn("quick", compute=True, compute_min_cu_fraction=0.5, seed=9)
    result = fn(Gpu())
    assert fn.level == "quick" and fn.compute is True
    assert _stages(order) == ["quick", "compute"]
    assert all(device == 3 for _, device, _ in order)  # one ordinal for all stages
    assert order[1][2] == {"seed": 9, "min_cu_fraction": 0.5}
    assert result == dict(GOOD_QUICK, compute=GOOD_COMPUTE)


def test_deep_plus_compute_runs_quick_compute_integrity(monkeypatch):
    order = _patch_probe(monkeypatch, GOOD_QUICK, GOOD_COMPUTE, GOOD_INTEGRITY)
    fn = probe_mod.make_probe_fn("deep", vram_bytes=64 << 20, compute=True)
    result = fn(Gpu())
    assert _stages(order) == ["quick", "compute", "integrity"]
    assert order[2][2]["vram_bytes"] == 64 << 20
    assert result["ok"] is True
    assert result["compute"] == GOOD_COMPUTE and result["integrity"] == GOOD_INTEGRITY


@pytest.mark.parametrize("level", ["quick", "deep"])
def test_stops_after_failed_quick(monkeypatch, level):
    order = _patch_probe(monkeypatch, {"ok": False, "rc": -2, "msg": "mfma"}, GOOD_COMPUTE,
                         GOOD_INTEGRITY)
    result = probe_mod.make_probe_fn(level, compute=True)(Gpu())
    assert _stages(order) == ["quick"]
    assert result == {"ok": False, "rc": -2, "msg": "mfma"}


@pytest.mark.parametrize("level", ["quick", "deep"])
def test_stops_after_failed_compute(monkeypatch, level):
    order = _patch_probe(monkeypatch, GOOD_QUICK, BAD_COMPUTE, GOOD_INTEGRITY)
    result = probe_mod.make_probe_fn(level, compute=True)(Gpu())
    assert _stages(order) == ["quick", "compute"]
    assert result["ok"] is False and result["msg"] == BAD_COMPUTE["msg"]
    assert result["compute"] == BAD_COMPUTE and "integrity" not in result
    assert result["mfma_f32_exact"] is True  # quick fields kept


def test_deep_plus_compute_failed_integrity(monkeypatch):
    order = _patch_probe(monkeypatch, GOOD_QUICK, GOOD_COMPUTE, BAD_INTEGRITY)
    result = probe_mod.make_probe_fn("deep", compute=True)(Gpu())
    assert _stages(order) == ["quick", "compute", "integrity"]
    assert result["ok"] is False and result["msg"] == BAD_INTEGRITY["msg"]
    assert result["compute"] == GOOD_COMPUTE and result["integrity"] == BAD_INTEGRITY


def test_run_compute_names_tests_and_builds_opts():
    opts = probe_mod._compute_opts(grid_blocks=8, lds_bytes=1024, iters=3, max_rounds=2,
                                   seed=-1, min_cu_fraction=0.25, selftest_mode=1,
                                   selftest_test="mfma_bf16", selftest_elem=999, selftest_bit=30,
                                   selftest_key=0x54700)
    assert (opts.grid_blocks, opts.lds_bytes, opts.iters, opts.max_rounds) == (8, 1024, 3, 2)
    assert opts.seed == 0xFFFFFFFF and opts.min_cu_fraction == 0.25
    assert (opts.selftest_mode, opts.selftest_test, opts.selftest_elem) == (1, 2, 999)
    assert (opts.selftest_bit, opts.selftest_key) == (30, 0x54700)
    zero = probe_mod._compute_opts()
    assert bytes(zero) == bytes(ctypes.sizeof(zero))  # every default is 0
    plant = probe_mod._compute_opts(selftest_mode=3, selftest_test="lds", selftest_elem=1023,
                                    selftest_span=2, selftest_pass=2, selftest_bit=31)
    assert (plant.selftest_mode, plant.selftest_test, plant.selftest_elem) == (3, 3, 1023)
    assert (plant.selftest_span, plant.selftest_pass, plant.selftest_bit) == (2, 2, 31)
    assert probe_mod._compute_opts(selftest_span=0xFFFFFFFF).selftest_span == 0xFFFFFFFF


def test_plant_fields_sit_between_the_key_and_the_floor():
    """The two new options fill the eight bytes before min_cu_fraction: no
    padding appears, and every older field keeps its offset."""
    opts = probe_mod.CroComputeOpts
    assert (opts.selftest_key.offset, opts.selftest_span.offset, opts.selftest_pass.offset,
            opts.min_cu_fraction.offset, ctypes.sizeof(opts)) == (36, 40, 44, 48, 56)


class FakeProbeLib:
    """Records what the wrappers hand to the library's test entries."""

    def __init__(self):
        self.calls = []

    def cro_probe_compute_tiles(self, device, opts, e32, e8, e16, res, buf, cap):
        self.calls.append(("tiles", device, opts._obj, (e32, e8, e16), cap))
        res._obj.rounds, res._obj.grid_blocks, res._obj.ok = 2, 3, 1
        for i in range(min(2 * 3 * 4, cap)):
            buf[i].valid, buf[i].first_bad = 1, i
        return 0

    def cro_probe_compute_lds_dump(self, device, grid, lds_bytes, seed, invert, elem, span, bit,
                                   out, guard):
        self.calls.append(("dump", device, grid, lds_bytes, seed, invert, elem, span, bit))
        words = (ctypes.c_uint * (grid * lds_bytes // 4)).from_address(out)
        for i in range(len(words)):
            words[i] = 7 * i
        guard._obj.value = 5
        return self.rc

    rc = 0


def test_run_compute_records_hands_on_the_callers_tiles(monkeypatch):
    fake = FakeProbeLib()
    monkeypatch.setattr(probe_mod, "load_library", lambda required=None: fake)
    e8 = np.arange(256, dtype=np.int32).reshape(16, 16)
    e16 = np.arange(1024, dtype=np.float32).reshape(32, 32)
    res, records = probe_mod.run_compute_records(2, tiles={"i8": e8, "bf16": e16},
                                                 grid_blocks=3, max_rounds=2, seed=9)
    (name, device, opts, tiles, cap), = fake.calls
    assert (name, device, cap) == ("tiles", 2, 3 * 4 * 2)
    assert (opts.grid_blocks, opts.max_rounds, opts.seed) == (3, 2, 9)
    assert tiles[0] is None  # f32: the cached tile
    assert np.array_equal(np.ctypeslib.as_array((ctypes.c_int * 256).from_address(tiles[1])),
                          e8.ravel())
    assert np.array_equal(np.ctypeslib.as_array((ctypes.c_float * 1024).from_address(tiles[2])),
                          e16.ravel())
    assert res["rounds"] == 2 and len(records) == 24
    assert records["first_bad"].tolist() == list(range(24))
    # no tiles: three null pointers
    probe_mod.run_compute_records(0, grid_blocks=1)
    assert fake.calls[-1][3] == (None, None, None)
    # a tile of the wrong type or size never reaches the library
    for bad in ({"f32": e8}, {"i8": e8[:8]}, {"bf16": e16.astype(np.float64)}, {"f16": e16}):
        with pytest.raises(ValueError):
            probe_mod.run_compute_records(0, tiles=bad)
    assert len(fake.calls) == 2


def test_compute_lds_dump_builds_its_arguments(monkeypatch):
    fake = FakeProbeLib()
    monkeypatch.setattr(probe_mod, "load_library", lambda required=None: fake)
    words, guard_bad = probe_mod.compute_lds_dump(1, 3, 1024, seed=-1, invert=True, plant_elem=2,
                                                  plant_span=5, plant_bit=7)
    assert fake.calls == [("dump", 1, 3, 1024, 0xFFFFFFFF, 1, 2, 5, 7)]
    assert words.shape == (3, 256) and words.dtype == np.uint32 and guard_bad == 5
    assert np.array_equal(words.ravel(), 7 * np.arange(768))  # block-major
    probe_mod.compute_lds_dump(0, 1, 16)
    assert fake.calls[-1] == ("dump", 0, 1, 16, 0, 0, 0, 0, 0)
    fake.rc = -10
    with pytest.raises(RuntimeError, match="rc=-10"):
        probe_mod.compute_lds_dump(0, 1, 16)


# -- which wave verifies which LDS word -----------------------------------------------------


def _walk_verify(lds_words):
    """The kernel's verify loop, index for index (coverage.hip): the wave that
    loads each word, and how often each word is loaded."""
    n4 = lds_words >> 2
    owner = np.full(lds_words, -1)
    loads = np.zeros(lds_words, dtype=int)
    for tid in range(256):
        lane, wave = tid & 63, tid >> 6
        v0 = tid - lane
        while v0 < n4:
            v = v0 + lane
            if v < n4:
                owner[4 * v:4 * v + 4] = wave
                loads[4 * v:4 * v + 4] += 1
            v0 += 256
    return owner, loads


def _walk_plant(lds_words, elem, span):
    """The kernel's plant loop: for each word stored, the storing thread."""
    lo, hi = elem, elem + span
    stores = {}
    for tid in range(256):
        v = ((lo >> 2) & ~255) | (tid ^ 128)
        while (v << 2) < hi:
            for w in range(v << 2, (v << 2) + 4):
                if lo <= w < hi:
                    assert w not in stores and w < lds_words
                    stores[w] = tid
            v += 256
    return stores


@pytest.mark.parametrize("lds_bytes", [16, 1024, 4096 + 16, 163840])
def test_lds_wave_expectations_agree_with_a_walk_of_the_kernels_loops(lds_bytes):
    lds_words = lds_bytes // 4
    owner, loads = _walk_verify(lds_words)
    assert np.all(loads == 1)  # every word verified, once
    assert np.array_equal(owner, probe_mod.lds_verify_wave(np.arange(lds_words)))
    plants = [(0, 1), (lds_words - 1, 1), (0, lds_words)]
    plants += [(e, 2) for e in (3, 255, 1023) if e + 2 <= lds_words]
    plants += [(2, 5)] if lds_words >= 7 else []
    for elem, span in plants:
        counts, firsts = probe_mod.lds_plant_per_wave(elem, span)
        words = np.arange(elem, elem + span)
        for wave in range(4):
            mine = words[owner[words] == wave]
            assert counts[wave] == mine.size, (elem, span, wave)
            assert firsts[wave] == (mine.min() if mine.size else NONE32), (elem, span, wave)
        # each planted word is stored once, in bounds, by a thread of another
        # wave than the one that verifies it
        stores = _walk_plant(lds_words, elem, span)
        assert sorted(stores) == words.tolist(), (elem, span)
        for w, tid in stores.items():
            assert tid >> 6 != owner[w], (elem, span, w)


# -- probe_via_exec -----------------------------------------------------------------------


class RecordingExec:
    def __init__(self, out='{"ok": true}'):
        self.argvs = []
        self.out = out

    def run(self, node, argv, timeout=None):
        self.argvs.append(list(argv))
        return 0, self.out, ""


def test_exec_probe_argv_with_and_without_compute():
    ex = RecordingExec('{"ok": true, "compute": {"ok": true}}')
    base = ["croagent", "probe", "--bdf", "0000:05:00.0"]
    probe_mod.probe_via_exec(ex, "n0", Gpu())
    probe_mod.probe_via_exec(ex, "n0", Gpu(), compute=False, compute_min_cu_fraction=0.9)
    out = probe_mod.probe_via_exec(ex, "n0", Gpu(), compute=True)
    assert out["compute"]["ok"] is True
    probe_mod.probe_via_exec(ex, "n0", Gpu(), compute=True, compute_min_cu_fraction=0.9)
    probe_mod.probe_via_exec(ex, "n0", Gpu(), level="deep", vram_mib=64, compute=True)
    probe_mod.make_exec_probe_fn(ex, "n0", argv_prefix_fn=lambda: ["chroot", "/d"],
                                 compute=True, compute_min_cu_fraction=1)(Gpu())
    probe_mod.make_exec_probe_fn(ex, "n0")(Gpu())
    assert ex.argvs == [
        base,
        base,
        base + ["--compute"],
        base + ["--compute", "--compute-min-cu-fraction", "0.9"],
        base + ["--deep", "--vram-mib", "64", "--compute"],
        ["chroot", "/d"] + base + ["--compute", "--compute-min-cu-fraction", "1.0"],
        base,
    ]


# -- controller ---------------------------------------------------------------------------


def _attach(world, probe_result):
    make_node(world.client, "node0")
    world.client.create(make_resource("gpu-1"))
    world.resource_rec.node_ops.health_probe = lambda node, device_id: probe_result
    world.resource_rec.reconcile("gpu-1")  # None → Attaching


def _online_message(world):
    world.recorder.flush(timeout=10)
    events = [e for e in world.client.list(Event) if e.reason == "Online"]
    assert len(events) == 1
    return events[0].message


def test_controller_refuses_online_on_compute_failure(mock_world):
    probe = dict(GOOD_QUICK, ok=False, compute=BAD_COMPUTE)
    _attach(mock_world, probe)
    metrics = mock_world.resource_rec.metrics
    counter = metrics.probe_compute_failures_total.labels(test="mfma_i8")
    integrity_counter = metrics.probe_integrity_failures_total.labels(stage="unknown")
    before, integrity_before = counter._value.get(), integrity_counter._value.get()
    with pytest.raises(FabricError):
        mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Attaching"
    assert got.status.error.startswith(
        "gfx950 health probe failed: compute stage mfma_i8 xcd=5 se=2 cu=7 simd=3 "
        "bits_bad=0x00400000 cus_bad=1"
    ), got.status.error
    assert counter._value.get() == before + 1
    assert integrity_counter._value.get() == integrity_before


def test_controller_online_event_carries_compute_summary(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, compute=GOOD_COMPUTE))
    mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Online"
    assert _online_message(mock_world) == (
        f"device {got.status.device_id} online with CDI spec"
        "; probe: mfma_exact=True hbm=4000 GB/s"
        "; compute: 256/256 CUs, 1024 SIMDs, 1.2 ms"
    )


def test_controller_online_event_compute_then_integrity(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, compute=GOOD_COMPUTE, integrity=GOOD_INTEGRITY))
    mock_world.resource_rec.reconcile("gpu-1")
    message = _online_message(mock_world)
    assert message.index("; compute: 256/256 CUs") < message.index("; integrity: vram 1.00 GiB")


def test_controller_messages_unchanged_without_compute_key(mock_world):
    _attach(mock_world, dict(GOOD_QUICK))
    mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert _online_message(mock_world) == (
        f"device {got.status.device_id} online with CDI spec"
        "; probe: mfma_exact=True hbm=4000 GB/s"
    )


def test_controller_failure_message_unchanged_without_compute_key(mock_world):
    probe = dict(GOOD_QUICK, ok=False, msg="f32 MFMA mismatch vs host fmaf chain")
    _attach(mock_world, probe)
    with pytest.raises(FabricError):
        mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.error.startswith(f"gfx950 health probe failed: {probe}"), got.status.error


def test_metrics_reset_unregisters_compute_counter():
    from prometheus_client import REGISTRY

    from cro_amd.metrics import Metrics

    Metrics()
    assert "cro_probe_compute_failures" in REGISTRY._names_to_collectors
    Metrics._reset_for_tests()
    try:
        assert "cro_probe_compute_failures" not in REGISTRY._names_to_collectors
    finally:
        Metrics()  # later tests share the process-wide singleton


# -- entrypoint ---------------------------------------------------------------------------


def _parse(argv):
    from cro_amd.cmd.main import add_probe_arguments

    p = argparse.ArgumentParser()
    add_probe_arguments(p)
    return p.parse_args(argv)


def _clear_env(monkeypatch):
    for name in ("CRO_PROBE_LEVEL", "CRO_PROBE_COMPUTE", "CRO_PROBE_COMPUTE_MIN_CU_FRACTION"):
        monkeypatch.delenv(name, raising=False)


def test_entrypoint_compute_default_off(monkeypatch):
    from cro_amd.cmd.main import select_probe_fn

    _clear_env(monkeypatch)
    args = _parse([])
    assert args.probe_compute == "off" and args.probe_compute_min_cu_fraction == 0
    assert select_probe_fn(args) is probe_mod.probe_fn_for_nodeops


def test_entrypoint_flag_selects_compute(monkeypatch):
    from cro_amd.cmd.main import select_probe_fn

    _clear_env(monkeypatch)
    fn = select_probe_fn(_parse(["--probe-compute", "on",
                                 "--probe-compute-min-cu-fraction", "0.75"]))
    assert fn is not probe_mod.probe_fn_for_nodeops
    assert fn.level == "quick" and fn.compute is True
    order = _patch_probe(monkeypatch, GOOD_QUICK, GOOD_COMPUTE, GOOD_INTEGRITY)
    assert fn(Gpu())["compute"] == GOOD_COMPUTE
    assert _stages(order) == ["quick", "compute"]
    assert order[1][2]["min_cu_fraction"] == 0.75
    both = select_probe_fn(_parse(["--probe-level", "deep", "--probe-compute", "on"]))
    assert both.level == "deep" and both.compute is True
    with pytest.raises(SystemExit):
        _parse(["--probe-compute", "maybe"])


def test_entrypoint_env_selects_compute(monkeypatch):
    from cro_amd.cmd.main import select_probe_fn

    _clear_env(monkeypatch)
    monkeypatch.setenv("CRO_PROBE_COMPUTE", "on")
    monkeypatch.setenv("CRO_PROBE_COMPUTE_MIN_CU_FRACTION", "0.5")
    args = _parse([])
    assert args.probe_compute == "on" and args.probe_compute_min_cu_fraction == 0.5
    assert select_probe_fn(args).compute is True
    # the flag wins over the environment
    assert select_probe_fn(_parse(["--probe-compute", "off"])) is probe_mod.probe_fn_for_nodeops


# -- build ----------------------------------------------------------------------------------


def test_build_goes_stale_on_coverage_source_or_header(tmp_path, monkeypatch):
    from cro_amd.hip import build as hip_build

    names = {os.path.basename(p) for p in hip_build.ALL_SRCS + hip_build.ALL_HEADERS}
    assert names == {"probe.hip", "integrity.hip", "coverage.hip", "croprobe.h",
                     "cropattern.h", "crocoverage.h", "crointegrity.h", "crohost.h",
                     "cromfma.h"}
    assert all(os.path.exists(p) for p in hip_build.ALL_SRCS + hip_build.ALL_HEADERS)
    # build() and build_agent() look at the new files: stand-ins with chosen
    # mtimes, a hipcc that only records its command line
    lib, agent = tmp_path / "libcroprobe.so", tmp_path / "croagent"
    files = {}
    for name in ("probe.hip", "integrity.hip", "coverage.hip", "croprobe.h", "cropattern.h",
                 "crocoverage.h", "crointegrity.h", "crohost.h", "cromfma.h", "croagent.cpp"):
        files[name] = tmp_path / name
        files[name].write_text("")
        os.utime(files[name], (100, 100))
    for out in (lib, agent):
        out.write_text("")
        os.utime(out, (200, 200))
    srcs = [str(files[n]) for n in ("probe.hip", "integrity.hip")]
    hdrs = [str(files[n]) for n in ("croprobe.h", "cropattern.h")]
    monkeypatch.setattr(hip_build, "SRCS", srcs)
    monkeypatch.setattr(hip_build, "HEADERS", hdrs)
    monkeypatch.setattr(hip_build, "COVERAGE_SRC", str(files["coverage.hip"]))
    monkeypatch.setattr(hip_build, "COVERAGE_HEADER", str(files["crocoverage.h"]))
    monkeypatch.setattr(hip_build, "ALL_SRCS", srcs + [str(files["coverage.hip"])])
    internal = [str(files[n]) for n in ("crohost.h", "cromfma.h")]
    monkeypatch.setattr(hip_build, "INTERNAL_HEADERS", internal)
    monkeypatch.setattr(hip_build, "INTEGRITY_HEADER", str(files["crointegrity.h"]))
    monkeypatch.setattr(hip_build, "ALL_HEADERS",
                        hdrs + [str(files["crocoverage.h"]), str(files["crointegrity.h"])]
                        + internal)
    monkeypatch.setattr(hip_build, "OUT", str(lib))
    monkeypatch.setattr(hip_build, "AGENT_SRC", str(files["croagent.cpp"]))
    monkeypatch.setattr(hip_build, "AGENT_OUT", str(agent))
    commands = []

    def fake_run(argv, check=True):
        commands.append(argv)
        out = argv[argv.index("-o") + 1]
        os.utime(out, (400, 400))

    monkeypatch.setattr(hip_build.subprocess, "run", fake_run)
    hip_build.build()
    assert commands == []  # everything up to date
    for newer, want_lib in (("coverage.hip", True), ("crocoverage.h", True),
                            ("crointegrity.h", True), ("crohost.h", True), ("cromfma.h", True)):
        for out in (lib, agent):
            os.utime(out, (200, 200))
        os.utime(files[newer], (300, 300))
        commands.clear()
        hip_build.build()
        outs = [c[c.index("-o") + 1] for c in commands]
        assert outs == [str(lib), str(agent)], (newer, commands)
        assert str(files["coverage.hip"]) in commands[0]  # compiled into the library
        os.utime(files[newer], (100, 100))
