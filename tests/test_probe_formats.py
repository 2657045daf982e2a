"""CPU tests of the matrix-format probe stage: the decode tables, packers,
inputs, expected tiles and aggregation of croformats.h against their numpy
mirrors (through a small host program built with the host C++ compiler, also
under the address and undefined-behaviour sanitizers: no HIP, no GPU), the
tables against torch's CPU dtypes, the exactness bounds, the C structs
against their ctypes mirrors, the kernel's assembly, and the plumbing from
the operator flags down to the agent."""

import argparse
import ctypes
import json
import logging
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cro_amd.api.v1alpha1.types import ComposableResource, Event
from cro_amd.fabric.base import FabricError
from cro_amd.hip import build as hip_build
from cro_amd.nodeops import formats as F
from cro_amd.nodeops import probe as probe_mod
from tests.conftest import make_node, make_resource

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(REPO, "cro_amd", "hip")
AGENT = os.path.join(REPO, "cro_amd", "agent", "croagent")
SEEDS = (0, 1, 0xDEADBEEF)
TESTS = list(range(len(F.FORMATS_TESTS)))


def _host_cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    pytest.fail("no host C++ compiler (c++/g++/clang++) on PATH")


def _build(tmp_path, name, source, extra=()):
    src = tmp_path / f"{name}.cpp"
    src.write_text(source)
    exe = tmp_path / name
    subprocess.run(
        [_host_cxx(), "-std=c++17", "-O1", "-ffp-contract=off", *extra, f"-I{HIP_DIR}", str(src),
         "-o", str(exe)],
        check=True, capture_output=True, text=True,
    )
    return str(exe)


# -- the header against the numpy mirrors -------------------------------------------------

FORMATS_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "croformats.h"

static void hex(const char* tag, const void* data, size_t n) {
  printf("%s ", tag);
  for (size_t i = 0; i < n; ++i) printf("%02x", ((const unsigned char*)data)[i]);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "tables")) {
    for (int fmt = 0; fmt <= CRO_FMT_F16; ++fmt) {
      const int n = 1 << cro_fmt_bits(fmt);
      std::vector<double> v(n);
      for (int c = 0; c < n; ++c) v[c] = cro_fmt_decode(fmt, (uint32_t)c);
      char tag[16];
      snprintf(tag, sizeof(tag), "fmt%d", fmt);
      hex(tag, v.data(), n * sizeof(double));
    }
    float t[256];
    printf("table_n %d %d %d\n", cro_fmt_table(CRO_FMT_E4M3, t), cro_fmt_table(CRO_FMT_E2M3, t),
           cro_fmt_table(CRO_FMT_E2M1, t));
    double s[256];
    for (int e = 0; e < 256; ++e) s[e] = cro_fmt_scale((uint32_t)e);
    hex("scale", s, sizeof(s));
    uint16_t h[511];
    for (int m = -255; m <= 255; ++m) h[m + 255] = cro_fmt_f16_of_sixteenths(m);
    hex("f16", h, sizeof(h));
    return 0;
  }
  if (!strcmp(argv[1], "inputs")) {
    const unsigned seed = (unsigned)strtoul(argv[2], nullptr, 0);
    static CroFmtInputs in;
    static uint32_t words[2 * CRO_FMT_MAX_ELEMS];
    static uint16_t back[CRO_FMT_MAX_OPERAND];
    for (int t = 0; t < CRO_FMT_TESTS; ++t) {
      const CroFmtTestDesc* d = cro_fmt_test(t);
      cro_fmt_make(t, seed, &in);
      const int n = d->m * d->k, ns = d->m * (d->k / 32);
      printf("test %d %s m %d k %d kstep %d kconst %d elems %d sel %d %d\n", t, d->name, d->m,
             d->k, d->kstep, cro_fmt_k(t), cro_fmt_elems(t), d->op_sel_a, d->op_sel_b);
      hex("codes_a", in.codes_a, n * 2);
      hex("codes_b", in.codes_b, n * 2);
      hex("val_a", in.val_a, n * sizeof(double));
      hex("val_b", in.val_b, n * sizeof(double));
      hex("scale_a", in.scale_a, ns);
      hex("scale_b", in.scale_b, ns);
      hex("packed_a", in.packed_a, d->m * cro_fmt_row_bytes(d->fmt_a, d->k));
      hex("packed_b", in.packed_b, d->m * cro_fmt_row_bytes(d->fmt_b, d->k));
      const int nw = cro_fmt_expected(&in, words);
      hex("expected", words, nw * 4);
      printf("quanta %.17g\n", cro_fmt_abs_quanta(&in));
      if (t != CRO_FMT_TEST_F64) {
        cro_fmt_unpack(d->fmt_a, in.packed_a, n, back);
        printf("roundtrip %d\n", memcmp(back, in.codes_a, n * 2) == 0);
      }
    }
    return 0;
  }
  if (!strcmp(argv[1], "aggregate")) {
    // records on stdin: xcc_id hw_id fail_mask n_bad first_bad bits_bad valid
    std::vector<CroFormatsRecord> recs;
    CroFormatsRecord r;
    memset(&r, 0, sizeof(r));
    while (scanf("%u %u %u %u %u %u %u", &r.xcc_id, &r.hw_id, &r.fail_mask, &r.n_bad,
                 &r.first_bad, &r.bits_bad, &r.valid) == 7)
      recs.push_back(r);
    CroFormatsAgg a;
    cro_formats_aggregate(recs.data(), recs.size(), &a);
    printf("{\"waves_run\":%llu,\"waves_bad\":%llu,", a.waves_run, a.waves_bad);
    for (int t = 0; t < CRO_FMT_TESTS; ++t)
      printf("\"bad_%s\":%llu,", cro_fmt_test(t)->name, a.bad[t]);
    printf("\"first_bad_index\":%lld,\"cus_seen\":%d,\"xcds_seen\":%d,\"simds_seen\":%d,"
           "\"cus_bad\":%d,\"xcd\":%d,\"se\":%d,\"sh\":%d,\"cu\":%d,\"simd\":%d,"
           "\"first_fail_mask\":%u,\"n_bad\":%u,\"first_bad\":%u,\"bits_bad\":%u,"
           "\"name\":\"%s\"}\n",
           a.first_bad_index, a.cus_seen, a.xcds_seen, a.simds_seen, a.cus_bad, a.xcd, a.se,
           a.sh, a.cu, a.simd, a.first_fail_mask, a.n_bad, a.first_bad, a.bits_bad,
           cro_fmt_test_name(a.first_fail_mask));
    return 0;
  }
  return 2;
}
"""


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def formats_exe(request, tmp_path_factory):
    """The host program, plain and under the address and undefined-behaviour
    sanitizers (a stand-alone program: it needs nothing preloaded)."""
    extra = () if request.param == "plain" else (
        "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    return _build(tmp_path_factory.mktemp(f"formats_{request.param}"), "formats_main",
                  FORMATS_MAIN, extra)


def _run(exe, *args, stdin=None):
    proc = subprocess.run([exe, *args], input=stdin, capture_output=True, text=True)
    assert proc.returncode == 0, (proc.returncode, proc.stderr[-3000:])
    return proc.stdout


def _parse_hex(out):
    blocks, current = [], None
    for line in out.splitlines():
        tag, _, rest = line.partition(" ")
        if tag == "test":
            current = {"head": rest.split()}
            blocks.append(current)
        elif current is not None:
            current[tag] = rest
        else:
            blocks.append({tag: rest})
    return blocks


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_decode_tables_scales_and_f16_match_the_header(formats_exe):
    lines = dict(line.split(" ", 1) for line in _run(formats_exe, "tables").splitlines())
    for fmt in (F.E4M3, F.E5M2, F.E2M3, F.E3M2, F.E2M1, F.F16):
        got = np.frombuffer(bytes.fromhex(lines[f"fmt{fmt}"]), dtype=np.float64)
        want = F.decode_table(fmt)
        assert got.size == 1 << F.FORMAT_BITS[fmt]
        assert np.array_equal(got, want, equal_nan=True), fmt
        real = ~np.isnan(want)
        assert np.array_equal(np.signbit(got[real]), np.signbit(want[real]))  # the two zeros
    assert lines["table_n"].split() == ["256", "64", "16"]
    scale = np.frombuffer(bytes.fromhex(lines["scale"]), dtype=np.float64)
    assert np.array_equal(scale, F.scale_value(np.arange(256)), equal_nan=True)
    f16 = np.frombuffer(bytes.fromhex(lines["f16"]), dtype=np.uint16)
    assert np.array_equal(f16, F.f16_of_sixteenths(np.arange(-255, 256)))
    assert np.array_equal(f16.view(np.float16).astype(np.float64), np.arange(-255, 256) / 16.0)


@pytest.mark.parametrize("seed", SEEDS)
def test_inputs_packers_and_expected_tiles_match_the_header(formats_exe, seed):
    blocks = _parse_hex(_run(formats_exe, "inputs", str(seed)))
    assert len(blocks) == len(TESTS)
    for idx, block in enumerate(blocks):
        t = F.FORMATS_TABLE[idx]
        head = block["head"]
        assert head[:2] == [str(idx), t.name]
        assert [int(head[i]) for i in (3, 5, 7, 9, 11)] == [t.m, t.k, t.kstep, t.k, t.elems]
        assert [int(head[13]), int(head[14])] == [t.op_sel_a, t.op_sel_b]
        inp = F.formats_inputs(idx, seed)
        for name, dtype in (("codes_a", np.uint16), ("codes_b", np.uint16),
                            ("val_a", np.float64), ("val_b", np.float64),
                            ("scale_a", np.uint8), ("scale_b", np.uint8)):
            got = np.frombuffer(bytes.fromhex(block[name]), dtype=dtype)
            assert _same(got, inp[name].reshape(-1).astype(dtype)), (t.name, name)
        for name in ("packed_a", "packed_b"):
            got = np.frombuffer(bytes.fromhex(block[name]), dtype=np.uint8)
            assert _same(got, np.ascontiguousarray(inp[name]).reshape(-1).view(np.uint8)), name
        want = F.formats_expected(idx, seed)
        got = np.frombuffer(bytes.fromhex(block["expected"]), dtype=want.dtype)
        assert _same(got, want.reshape(-1)), t.name
        assert float(block["quanta"]) == F.formats_abs_quanta(idx, seed)
        if idx != 6:
            assert block["roundtrip"] == "1"
            assert np.array_equal(F.unpack_codes(t.fmt_a, inp["packed_a"], t.k), inp["codes_a"])


def _records(rows):
    dtype = np.dtype([(n, np.uint32) for n, _ in F.CroFormatsRecord._fields_])
    out = np.zeros(len(rows), dtype=dtype)
    for i, row in enumerate(rows):
        for key, value in row.items():
            out[i][key] = value
    return out


def _hw(se, sh, cu, simd, slot=0):
    return (se << 13) | (sh << 12) | (cu << 8) | (simd << 4) | slot


AGG_CASES = {
    "clean": [dict(xcc_id=x, hw_id=_hw(s, 0, c, d), valid=1)
              for x in range(8) for s in range(4) for c in range(3) for d in range(4)],
    "unwritten_and_three_simds": [dict(xcc_id=1, hw_id=_hw(2, 1, 5, d), valid=1)
                                  for d in range(3)] + [dict(valid=0, fail_mask=9)],
    "two_bad": [dict(xcc_id=0, hw_id=_hw(0, 0, 1, 0), valid=1),
                dict(xcc_id=5, hw_id=_hw(2, 0, 7, 3, 9), valid=1, fail_mask=0x48, n_bad=3,
                     first_bad=200, bits_bad=0x400000),
                dict(xcc_id=5, hw_id=_hw(2, 0, 7, 1), valid=1, fail_mask=0x01, n_bad=1,
                     first_bad=0, bits_bad=1),
                dict(xcc_id=6, hw_id=_hw(1, 1, 2, 2), valid=1, fail_mask=0x7F, n_bad=9,
                     first_bad=4, bits_bad=0xFFFFFFFF)],
    "empty": [],
}


@pytest.mark.parametrize("case", sorted(AGG_CASES))
def test_aggregation_of_hand_made_records_matches_the_header(formats_exe, case):
    records = _records(AGG_CASES[case])
    text = "".join(
        " ".join(str(int(r[k])) for k in ("xcc_id", "hw_id", "fail_mask", "n_bad", "first_bad",
                                          "bits_bad", "valid")) + "\n" for r in records)
    got = json.loads(_run(formats_exe, "aggregate", stdin=text))
    want = F.aggregate_formats_records(records)
    assert got.pop("name") == F.formats_test_name(want["first_fail_mask"])
    assert got == want
    if case == "two_bad":
        assert (want["waves_bad"], want["cus_bad"], want["first_bad_index"]) == (3, 2, 1)
        assert (want["xcd"], want["se"], want["cu"], want["simd"]) == (5, 2, 7, 3)
        assert want["bad_mx_fp8"] == 2 and want["bad_mfma_f64"] == 2 and want["bad_mfma_f16"] == 2
        assert F.formats_test_name(0x48) == "mx_fp8"
    if case == "clean":
        assert (want["cus_seen"], want["xcds_seen"], want["simds_seen"]) == (96, 8, 384)


# -- the tables against torch ----------------------------------------------------------------


def test_decode_tables_match_torch():
    import torch

    codes = torch.arange(256, dtype=torch.uint8)
    for fmt, dtype in ((F.E4M3, torch.float8_e4m3fn), (F.E5M2, torch.float8_e5m2)):
        want = codes.view(dtype).to(torch.float64).numpy()
        assert np.array_equal(F.decode_table(fmt), want, equal_nan=True), fmt
    want = codes.view(torch.float8_e8m0fnu).to(torch.float64).numpy()
    assert np.array_equal(F.scale_value(np.arange(256)), want, equal_nan=True)
    # the small formats, by their definition: OCP MX v1.0, no infinities or NaN
    assert sorted(set(np.abs(F.decode_table(F.E2M1)))) == [0, 0.5, 1, 1.5, 2, 3, 4, 6]
    assert np.abs(F.decode_table(F.E2M3)).max() == 7.5 and F.decode_table(F.E2M3)[1] == 0.125
    assert np.abs(F.decode_table(F.E3M2)).max() == 28.0 and F.decode_table(F.E3M2)[1] == 0.0625
    for fmt in (F.E2M1, F.E2M3, F.E3M2):
        assert np.isfinite(F.decode_table(fmt)).all()


# -- exact by construction ----------------------------------------------------------------------


def _code_set(fmt, e_lo, e_n):
    """The magnitudes a side's code set can take."""
    if fmt == F.F16:
        return np.arange(0, 256) / 16.0
    if fmt == F.F64:
        return np.array([0.0, 1.0, float((1 << 20) - 1)])
    ebits, mbits, _ = F._EBITS_MBITS_BIAS[fmt]
    codes = [(e << mbits) | m for e in range(e_lo, e_lo + e_n) for m in range(1 << mbits)]
    return np.abs(F.decode_table(fmt)[codes])


@pytest.mark.parametrize("idx", TESTS, ids=F.FORMATS_TESTS)
def test_exactness_bound_holds_in_the_worst_case_and_for_real_inputs(idx):
    """Worst case over the code set and the scale set: K times the largest
    product times the largest scale product, in quanta of the smallest, stays
    below 2^24 (2^53 for f64); every value is a whole number of quanta."""
    t = F.FORMATS_TABLE[idx]
    limit = 2.0 ** 53 if t.fmt_a == F.F64 else 2.0 ** 24
    mag_a, mag_b = _code_set(t.fmt_a, t.e_lo_a, t.e_n_a), _code_set(t.fmt_b, t.e_lo_b, t.e_n_b)
    for mag, q in ((mag_a, t.q_a), (mag_b, t.q_b)):
        assert np.array_equal(mag / q, np.round(mag / q)) and (mag[mag > 0] / q).min() >= 1
    spread = 2.0 ** (4 * t.scale_spread)  # largest over smallest scale product
    worst = t.k * (mag_a.max() / t.q_a) * (mag_b.max() / t.q_b) * spread
    assert worst < limit, (t.name, worst)
    table = {"mfma_f16": 4161600, "mfma_fp8": 230400, "mfma_bf8": 100352, "mx_fp8": 6881280,
             "mx_fp6": 6881280, "mx_fp4": 9437184, "mfma_f64": 64 * ((1 << 20) - 1) ** 2}
    assert worst == table[t.name]
    for seed in SEEDS:
        inp = F.formats_inputs(idx, seed)
        assert set(np.abs(inp["val_a"]).reshape(-1)) <= set(mag_a) or t.fmt_a == F.F64
        assert np.abs(inp["val_a"]).max() <= mag_a.max() and np.abs(inp["val_b"]).max() <= mag_b.max()
        if t.scaled:
            for side, base in (("scale_a", t.scale_base_a), ("scale_b", t.scale_base_b)):
                assert inp[side].min() >= base - t.scale_spread
                assert inp[side].max() <= base + t.scale_spread
                assert len(set(inp[side].reshape(-1))) == 2 * t.scale_spread + 1
        assert 0 < F.formats_abs_quanta(idx, seed) <= worst


@pytest.mark.parametrize("idx", [1, 2], ids=["mfma_fp8", "mfma_bf8"])
def test_non_scaled_8_bit_code_sets_span_twelve_bits(idx):
    """The non-scaled fp8 / bf8 instructions drop product bits further than 14
    below the largest product's leading bit (croformats.h): from that bit down
    to the quantum of the smallest product the code sets span 12."""
    t = F.FORMATS_TABLE[idx]
    mag_a, mag_b = _code_set(t.fmt_a, t.e_lo_a, t.e_n_a), _code_set(t.fmt_b, t.e_lo_b, t.e_n_b)
    largest = mag_a.max() * mag_b.max() / (t.q_a * t.q_b)
    assert int(np.floor(np.log2(largest))) + 1 == 12


@pytest.mark.parametrize("idx", TESTS, ids=F.FORMATS_TESTS)
def test_expected_tile_is_the_same_in_three_summation_orders(idx):
    t = F.FORMATS_TABLE[idx]
    for seed in SEEDS[:2]:
        inp = F.formats_inputs(idx, seed)
        want = F.formats_expected(idx, seed)
        g = t.k // 32
        wa = np.repeat(F.scale_value(inp["scale_a"]), 32, axis=1)
        wb = np.repeat(F.scale_value(inp["scale_b"]), 32, axis=1)
        terms = (inp["val_a"] * wa)[:, None, :] * (inp["val_b"] * wb)[None, :, :]
        orders = (np.arange(t.k), np.arange(t.k)[::-1],
                  np.random.default_rng(seed).permutation(t.k))
        for dtype in (np.float64,) + (() if t.fmt_a == F.F64 else (np.float32,)):
            for order in orders:
                acc = np.zeros((t.m, t.m), dtype=dtype)
                for kk in order:  # one rounding per step in the accumulator's type
                    acc = acc + terms[:, :, kk].astype(dtype)
                assert np.array_equal(acc.astype(want.dtype), want), (t.name, seed, dtype)
        assert not np.array_equal(want, want.T) and g >= 1


# -- struct layouts -------------------------------------------------------------------------------


def _struct_main():
    mirrors = {"CroFormatsOpts": F.CroFormatsOpts, "CroFormatsRecord": F.CroFormatsRecord}
    lines = ["#include <cstdio>", "#include <cstddef>", '#include "croformats.h"', "int main() {"]
    for name, mirror in mirrors.items():
        for field, _ in mirror._fields_:
            lines.append(f'  printf("{name} {field} %zu %zu\\n", offsetof({name}, {field}), '
                         f"sizeof((({name}*)0)->{field}));")
        lines.append(f'  printf("{name} sizeof %zu\\n", sizeof({name}));')
    agg = {n for n, _ in F.FORMATS_AGG_FIELDS}
    for field, _ in F.CroFormatsResult._fields_:
        if field.startswith("bad_"):
            i = F.FORMATS_TESTS.index(field[4:])
            path, size = f"agg.bad[{i}]", "sizeof(unsigned long long)"
            lines.append(f'  printf("CroFormatsResult {field} %zu %zu\\n", '
                         f"offsetof(CroFormatsResult, agg.bad) + {i} * {size}, {size});")
            continue
        path = f"agg.{field}" if field in agg else field
        lines.append(f'  printf("CroFormatsResult {field} %zu %zu\\n", '
                     f"offsetof(CroFormatsResult, {path}), "
                     f"sizeof(((CroFormatsResult*)0)->{path}));")
    lines.append('  printf("CroFormatsResult sizeof %zu\\n", sizeof(CroFormatsResult));')
    lines += ["  return 0;", "}"]
    return "\n".join(lines)


def test_formats_struct_layouts_match_ctypes(tmp_path):
    exe = _build(tmp_path, "struct_main", _struct_main(), ("-Wno-invalid-offsetof",))
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    mirrors = {"CroFormatsOpts": F.CroFormatsOpts, "CroFormatsRecord": F.CroFormatsRecord,
               "CroFormatsResult": F.CroFormatsResult}
    seen = 0
    for line in out.splitlines():
        name, field, *nums = line.split()
        mirror = mirrors[name]
        if field == "sizeof":
            assert ctypes.sizeof(mirror) == int(nums[0]), line
        else:
            desc = getattr(mirror, field)
            assert (desc.offset, desc.size) == (int(nums[0]), int(nums[1])), line
        seen += 1
    assert seen == 3 + sum(len(m._fields_) for m in mirrors.values())
    assert ctypes.sizeof(F.CroFormatsRecord) == 32


# -- the kernel's assembly ---------------------------------------------------------------------


@pytest.fixture(scope="module")
def stage_asm(tmp_path_factory):
    """formats.hip's device assembly with the library's flags; the text of
    the stage kernel."""
    out = tmp_path_factory.mktemp("formats_asm") / "formats.s"
    subprocess.run([hip_build.HIPCC, *hip_build.DEVICE_FLAGS, "-S", "--cuda-device-only",
                    hip_build.FORMATS_SRC, "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    match = re.search(r"^(_ZN\S*14formats_kernel\S*):[^\n]*\n(.*?)^\s*s_endpgm", text, re.S | re.M)
    assert match, "formats_kernel not found in the assembly"
    return match.group(2)


def test_stage_kernel_holds_all_seven_instructions(stage_asm):
    mfma = [line.strip() for line in stage_asm.splitlines() if line.strip().startswith("v_mfma")]

    def of(mnemonic):
        return [line for line in mfma if line.split()[0] == mnemonic]

    assert len(of("v_mfma_f32_16x16x32_f16")) == 2
    assert len(of("v_mfma_f32_16x16x32_fp8_fp8")) == 2
    assert len(of("v_mfma_f32_32x32x16_bf8_bf8")) == 2
    assert len(of("v_mfma_f64_16x16x4_f64")) == 16
    mx16 = of("v_mfma_scale_f32_16x16x128_f8f6f4")
    mx32 = of("v_mfma_scale_f32_32x32x64_f8f6f4")
    assert len(mx16) == 4 and len(mx32) == 2 and len(mfma) == 28
    fp8 = [line for line in mx16 if "cbsz" not in line]  # cbsz 0 is not printed
    fp4 = [line for line in mx16 if "cbsz:4" in line]
    assert len(fp8) == 2 and all(line.endswith("blgp:1") for line in fp8)
    assert len(fp4) == 2 and all(line.endswith("cbsz:4 blgp:4") for line in fp4)
    assert all(line.endswith("cbsz:2 blgp:3") for line in mx32)
    # op_sel a = bit 0 of op_sel / op_sel_hi element 0, op_sel b = element 1
    assert all("op_sel:[1,0,0] op_sel_hi:[0,1,0]" in line for line in fp8)   # a 1, b 2
    assert all("op_sel:[1,1,0] op_sel_hi:[1,0,0]" in line for line in fp4)   # a 3, b 1
    assert all("op_sel:" not in line and "op_sel_hi:[0,0,0]" in line for line in mx32)  # 0, 0
    # the second instruction of every check accumulates onto the first
    for group in (of("v_mfma_f32_16x16x32_f16"), fp8, fp4, mx32):
        assert sum(1 for line in group if re.search(r", 0(,| |$)", line)) == 1, group
    # no LDS traffic (the shuffles' lane exchanges touch no LDS memory), no
    # atomics, no spin
    assert not re.search(r"^\s*(ds_(?!bpermute|permute|swizzle)|global_atomic|flat_atomic|"
                         r"s_sleep|s_barrier)", stage_asm, re.M)


# -- plumbing ----------------------------------------------------------------------------------------


class Gpu:
    pci_bdf = "0000:05:00.0"


GOOD_QUICK = {"ok": True, "rc": 0, "mfma_f32_exact": True, "hbm_gbps": 4000.0, "msg": "ok"}
GOOD_STAGE = {
    "ok": True, "rc": 0, "cus_expected": 256, "cus_seen": 256, "xcds_seen": 8,
    "simds_seen": 1024, "rounds": 1, "waves_run": 1024, "waves_bad": 0, "cus_bad": 0,
    "failed_test": "", "gpu_ms": 0.134, "msg": "ok",
}
BAD_FORMATS = {
    "ok": False, "rc": -32, "cus_expected": 256, "cus_seen": 256, "xcds_seen": 8,
    "simds_seen": 1024, "rounds": 1, "waves_run": 1024, "waves_bad": 4, "cus_bad": 1,
    "failed_test": "mx_fp6", "xcd": 5, "se": 2, "sh": 0, "cu": 7, "simd": 3,
    "first_bad": 200, "bits_bad": 0x00400000, "n_bad": 16,
    "msg": "format mismatch in mx_fp6 at xcd=5 se=2 sh=0 cu=7 simd=3",
}
GOOD_INTEGRITY = {
    "ok": True, "rc": 0, "n_bad": 0, "failed_stage": "", "msg": "ok",
    "vram_passes": 2, "vram_bytes_verified": 2 << 30,
    "h2d_dma_bytes_verified": 256 << 20, "d2h_dma_bytes_verified": 256 << 20,
    "h2d_dma_gbps": 51.5, "d2h_dma_gbps": 49.0,
}


def _patch_probe(monkeypatch, quick=GOOD_QUICK, compute=GOOD_STAGE, formats=GOOD_STAGE,
                 integrity=GOOD_INTEGRITY):
    order = []

    def runner(name, result):
        def run(device=0, **kw):
            order.append((name, device, kw))
            return dict(result)
        return run

    monkeypatch.setattr(probe_mod, "hip_device_for_bdf", lambda bdf: 3)
    monkeypatch.setattr(probe_mod, "run_probe", runner("quick", quick))
    monkeypatch.setattr(probe_mod, "run_compute", runner("compute", compute))
    monkeypatch.setattr(F, "run_formats", runner("formats", formats))
    monkeypatch.setattr(probe_mod, "run_integrity", runner("integrity", integrity))
    return order


def _stages(order):
    return [name for name, _, _ in order]


def test_formats_off_returns_todays_hooks(monkeypatch):
    assert probe_mod.make_probe_fn("quick", formats=False) is probe_mod.probe_fn_for_nodeops
    order = _patch_probe(monkeypatch)
    fn = probe_mod.make_probe_fn("deep", compute=True, formats=False)
    assert fn(Gpu()) == dict(GOOD_QUICK, compute=GOOD_STAGE, integrity=GOOD_INTEGRITY)
    assert _stages(order) == ["quick", "compute", "integrity"] and not hasattr(fn, "formats")


def test_stage_order_and_result(monkeypatch):
    order = _patch_probe(monkeypatch)
    fn = probe_mod.make_probe_fn("deep", compute=True, formats=True, seed=9,
                                 formats_min_cu_fraction=0.5)
    result = fn(Gpu())
    assert _stages(order) == ["quick", "compute", "formats", "integrity"]
    assert all(device == 3 for _, device, _ in order)
    assert order[2][2] == {"seed": 9, "min_cu_fraction": 0.5}
    assert list(result)[-3:] == ["compute", "formats", "integrity"] and result["ok"] is True
    order.clear()
    quick = probe_mod.make_probe_fn("quick", formats=True)
    assert quick(Gpu()) == dict(GOOD_QUICK, formats=GOOD_STAGE) and quick.formats is True
    assert _stages(order) == ["quick", "formats"]


def test_stops_at_the_first_failing_stage(monkeypatch):
    fn = probe_mod.make_probe_fn("deep", compute=True, formats=True)
    order = _patch_probe(monkeypatch, quick={"ok": False, "rc": -2, "msg": "mfma"})
    assert fn(Gpu()) == {"ok": False, "rc": -2, "msg": "mfma"} and _stages(order) == ["quick"]
    order = _patch_probe(monkeypatch, compute=dict(GOOD_STAGE, ok=False, msg="c"))
    result = fn(Gpu())
    assert _stages(order) == ["quick", "compute"] and "formats" not in result
    order = _patch_probe(monkeypatch, formats=BAD_FORMATS)
    result = fn(Gpu())
    assert _stages(order) == ["quick", "compute", "formats"]
    assert result["ok"] is False and result["msg"] == BAD_FORMATS["msg"]
    assert result["formats"] == BAD_FORMATS and "integrity" not in result
    order = _patch_probe(monkeypatch, integrity=dict(GOOD_INTEGRITY, ok=False, msg="i"))
    result = fn(Gpu())
    assert _stages(order) == ["quick", "compute", "formats", "integrity"]
    assert result["msg"] == "i" and result["formats"] == GOOD_STAGE


def test_run_formats_builds_its_options(monkeypatch):
    seen = {}

    class Lib:
        @staticmethod
        def cro_formats_run(device, opts, res):
            o = ctypes.cast(opts, ctypes.POINTER(F.CroFormatsOpts)).contents
            seen.update({name: getattr(o, name) for name, _ in F.CroFormatsOpts._fields_})
            seen["device"] = device
            return -33

    monkeypatch.setattr(F, "load_formats_library", lambda required=None: Lib)
    out = F.run_formats(2, grid_blocks=3, iters=5, max_rounds=2, seed=-1, min_cu_fraction=0.25,
                        selftest_mode=1, selftest_test="mx_fp4", selftest_also="mfma_f16",
                        selftest_elem=7, selftest_bit=30, selftest_key=0x50700)
    assert seen == {"device": 2, "grid_blocks": 3, "iters": 5, "max_rounds": 2,
                    "seed": 0xFFFFFFFF, "selftest_mode": 1, "selftest_test": 5,
                    "selftest_bit": 30, "selftest_elem": 7, "selftest_key": 0x50700,
                    "selftest_also": 1, "min_cu_fraction": 0.25}
    assert out["ok"] is False and out["rc"] == -33 and list(out)[:2] == ["ok", "rc"]
    assert [k for k in out if k.startswith("bad_")] == [f"bad_{n}" for n in F.FORMATS_TESTS]
    with pytest.raises(TypeError):
        F.run_formats(0, lds_bytes=16)


def test_loader_without_the_library(monkeypatch, tmp_path):
    monkeypatch.setattr(F, "_lib", None)
    monkeypatch.setattr(F, "_LIB_PATH", str(tmp_path / "libcroformats.so"))
    assert F.load_formats_library(required=False) is None
    with pytest.raises(RuntimeError, match="libcroformats.so missing"):
        F.load_formats_library(required=True)
    with pytest.raises(RuntimeError):
        F.run_formats(0)  # never a silent pass


class RecordingExec:
    def __init__(self, stdout):
        self.stdout, self.argvs = stdout, []

    def run(self, node, argv, timeout=0):
        self.argvs.append(list(argv))
        return 0, self.stdout, ""


def test_exec_probe_argv_with_and_without_formats():
    ex = RecordingExec('{"ok": true, "formats": {"ok": true}}')
    base = ["croagent", "probe", "--bdf", "0000:05:00.0"]
    probe_mod.probe_via_exec(ex, "n0", Gpu())
    probe_mod.probe_via_exec(ex, "n0", Gpu(), formats=False, formats_min_cu_fraction=0.9)
    assert probe_mod.probe_via_exec(ex, "n0", Gpu(), formats=True)["formats"]["ok"] is True
    probe_mod.probe_via_exec(ex, "n0", Gpu(), formats=True, formats_min_cu_fraction=0.9)
    probe_mod.probe_via_exec(ex, "n0", Gpu(), level="deep", vram_mib=64, compute=True,
                             formats=True)
    probe_mod.make_exec_probe_fn(ex, "n0", argv_prefix_fn=lambda: ["chroot", "/d"],
                                 formats=True, formats_min_cu_fraction=1)(Gpu())
    probe_mod.make_exec_probe_fn(ex, "n0", compute=True)(Gpu())
    assert ex.argvs == [
        base,
        base,
        base + ["--formats"],
        base + ["--formats", "--formats-min-cu-fraction", "0.9"],
        base + ["--deep", "--vram-mib", "64", "--compute", "--formats"],
        ["chroot", "/d"] + base + ["--formats", "--formats-min-cu-fraction", "1.0"],
        base + ["--compute"],
    ]


# -- controller -----------------------------------------------------------------------------------------


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


def test_controller_refuses_online_on_formats_failure(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, ok=False, compute=GOOD_STAGE, formats=BAD_FORMATS))
    metrics = mock_world.resource_rec.metrics
    counter = metrics.probe_formats_failures_total.labels(test="mx_fp6")
    compute_counter = metrics.probe_compute_failures_total.labels(test="unknown")
    before, compute_before = counter._value.get(), compute_counter._value.get()
    with pytest.raises(FabricError):
        mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Attaching"
    assert got.status.error.startswith(
        "gfx950 health probe failed: formats stage mx_fp6 xcd=5 se=2 cu=7 simd=3 "
        "bits_bad=0x00400000 cus_bad=1"
    ), got.status.error
    assert counter._value.get() == before + 1
    assert compute_counter._value.get() == compute_before


def test_controller_counts_the_coverage_floor(mock_world):
    floor = dict(GOOD_STAGE, ok=False, rc=-33, msg="coverage 3 of 256 CUs")
    _attach(mock_world, dict(GOOD_QUICK, ok=False, formats=floor))
    counter = mock_world.resource_rec.metrics.probe_formats_failures_total.labels(test="coverage")
    before = counter._value.get()
    with pytest.raises(FabricError):
        mock_world.resource_rec.reconcile("gpu-1")
    assert counter._value.get() == before + 1


def test_controller_online_event_carries_the_formats_clause(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, compute=dict(GOOD_STAGE, gpu_ms=1.234),
                             formats=GOOD_STAGE, integrity=GOOD_INTEGRITY))
    mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Online"
    assert _online_message(mock_world) == (
        f"device {got.status.device_id} online with CDI spec"
        "; probe: mfma_exact=True hbm=4000 GB/s"
        "; compute: 256/256 CUs, 1024 SIMDs, 1.2 ms"
        "; formats: 256/256 CUs, 1024 SIMDs, 0.1 ms"
        "; integrity: vram 1.00 GiB link 0.25 GiB verified, h2d 51.5 d2h 49.0 GB/s"
    )


def test_controller_messages_unchanged_without_a_formats_object(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, compute=dict(GOOD_STAGE, gpu_ms=1.234)))
    mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert _online_message(mock_world) == (
        f"device {got.status.device_id} online with CDI spec"
        "; probe: mfma_exact=True hbm=4000 GB/s"
        "; compute: 256/256 CUs, 1024 SIMDs, 1.2 ms"
    )


def test_metrics_reset_unregisters_the_formats_counter():
    from prometheus_client import REGISTRY

    from cro_amd.metrics import Metrics

    Metrics()
    assert "cro_probe_formats_failures" in REGISTRY._names_to_collectors
    Metrics._reset_for_tests()
    try:
        assert "cro_probe_formats_failures" not in REGISTRY._names_to_collectors
    finally:
        Metrics()  # later tests share the process-wide singleton


# -- operator flags ---------------------------------------------------------------------------------------


def _parse(argv):
    from cro_amd.cmd.main import add_probe_arguments

    p = argparse.ArgumentParser()
    add_probe_arguments(p)
    return p.parse_args(argv)


def _clear_env(monkeypatch):
    for name in ("CRO_PROBE_LEVEL", "CRO_PROBE_COMPUTE", "CRO_PROBE_COMPUTE_MIN_CU_FRACTION",
                 "CRO_PROBE_FORMATS", "CRO_PROBE_FORMATS_MIN_CU_FRACTION"):
        monkeypatch.delenv(name, raising=False)


def test_entrypoint_formats_default_off_passes_todays_keywords(monkeypatch):
    from cro_amd.cmd import main as main_mod

    _clear_env(monkeypatch)
    args = _parse([])
    assert args.probe_formats == "off" and args.probe_formats_min_cu_fraction == 0
    assert main_mod.select_probe_fn(args) is probe_mod.probe_fn_for_nodeops
    seen = {}
    monkeypatch.setattr(probe_mod, "make_probe_fn", lambda level, **kw: seen.update(kw))
    main_mod.select_probe_fn(_parse(["--probe-compute", "on"]))
    assert sorted(seen) == ["compute", "compute_min_cu_fraction", "link_bytes",
                            "link_floor_gbps", "vram_bytes"]


def test_entrypoint_flag_and_env_select_formats(monkeypatch):
    from cro_amd.cmd.main import select_probe_fn

    _clear_env(monkeypatch)
    fn = select_probe_fn(_parse(["--probe-formats", "on",
                                 "--probe-formats-min-cu-fraction", "0.75"]))
    assert fn.level == "quick" and fn.formats is True and fn.compute is False
    order = _patch_probe(monkeypatch)
    assert fn(Gpu())["formats"] == GOOD_STAGE and _stages(order) == ["quick", "formats"]
    assert order[1][2]["min_cu_fraction"] == 0.75
    with pytest.raises(SystemExit):
        _parse(["--probe-formats", "maybe"])
    monkeypatch.setenv("CRO_PROBE_FORMATS", "on")
    monkeypatch.setenv("CRO_PROBE_FORMATS_MIN_CU_FRACTION", "0.5")
    args = _parse([])
    assert args.probe_formats == "on" and args.probe_formats_min_cu_fraction == 0.5
    assert select_probe_fn(args).formats is True
    # the flag wins over the environment
    assert select_probe_fn(_parse(["--probe-formats", "off"])) is probe_mod.probe_fn_for_nodeops


def test_a_missing_library_warns_and_switches_the_stage_off(monkeypatch, caplog):
    from cro_amd.cmd.main import drop_unavailable_probe_stages, select_probe_fn

    _clear_env(monkeypatch)
    log = logging.getLogger("test-formats")
    args = _parse(["--probe-formats", "on"])
    monkeypatch.setattr(F, "load_formats_library", lambda required=None: object())
    with caplog.at_level(logging.INFO, logger="test-formats"):
        assert drop_unavailable_probe_stages(args, log) is False
    assert args.probe_formats == "on" and "matrix-format stage: on" in caplog.text
    caplog.clear()
    monkeypatch.setattr(F, "load_formats_library", lambda required=None: None)
    with caplog.at_level(logging.INFO, logger="test-formats"):
        assert drop_unavailable_probe_stages(args, log) is True
    assert args.probe_formats == "off"
    assert "matrix-format probe library unavailable; formats stage disabled" in caplog.text
    assert select_probe_fn(args) is probe_mod.probe_fn_for_nodeops

    def broken(required=None):
        raise OSError("cannot load")

    args = _parse(["--probe-formats", "on"])
    monkeypatch.setattr(F, "load_formats_library", broken)
    assert drop_unavailable_probe_stages(args, log) is True and args.probe_formats == "off"
    caplog.clear()
    assert drop_unavailable_probe_stages(_parse([]), log) is False and caplog.text == ""


# -- croagent ------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def agent():
    if not os.path.exists(AGENT) or not os.path.exists(hip_build.OUT):
        hip_build.build()
    if not os.path.exists(hip_build.FORMATS_OUT):
        hip_build.build_formats()
    return AGENT


def test_croagent_probe_formats_without_a_gpu_reports_the_quick_failure(agent):
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present: the GPU tests run the stage itself")
    run = subprocess.run([agent, "probe", "--formats", "--formats-min-cu-fraction", "0.5"],
                         capture_output=True, text=True, timeout=60)
    out = json.loads(run.stdout)
    assert run.returncode == 1 and out["ok"] is False and "formats" not in out, out
    plain = subprocess.run([agent, "probe"], capture_output=True, text=True, timeout=60)
    assert plain.stdout == run.stdout  # a stage that did not run leaves no trace


def test_croagent_probe_formats_without_the_library(agent, tmp_path, monkeypatch):
    """An agent built by the build's own recipe beside libcroprobe.so only:
    ``probe --formats`` names the library that is missing before anything
    runs, in the scrubs' shape."""
    (tmp_path / "agent").mkdir()
    (tmp_path / "hip").mkdir()
    lone = tmp_path / "agent" / "croagent"
    shutil.copy(hip_build.OUT, tmp_path / "hip" / "libcroprobe.so")
    monkeypatch.setattr(hip_build, "HIP_DIR", str(tmp_path / "hip"))
    monkeypatch.setattr(hip_build, "AGENT_OUT", str(lone))
    hip_build.build_agent(force=True)
    run = subprocess.run([str(lone), "probe", "--formats"], capture_output=True, text=True,
                         timeout=60)
    (line,) = run.stdout.strip().splitlines()
    out = json.loads(line)
    assert run.returncode == 1 and set(out) == {"ok", "rc", "msg"}, out
    assert out["ok"] is False and out["rc"] == -1
    assert out["msg"].startswith("libcroformats.so not available: ")
    shutil.copy(hip_build.FORMATS_OUT, tmp_path / "hip" / "libcroformats.so")
    again = subprocess.run([str(lone), "probe", "--formats"], capture_output=True, text=True,
                           timeout=60)
    assert "libcroformats.so not available" not in again.stdout


# -- build --------------------------------------------------------------------------------------------------


def test_build_formats_inputs_staleness_and_command(tmp_path, monkeypatch):
    inputs = [hip_build.FORMATS_SRC] + hip_build.FORMATS_HEADERS
    assert {os.path.basename(p) for p in inputs} == {
        "formats.hip", "croformats.h", "crohost.h", "cromfma.h", "crocoverage.h"}
    assert all(os.path.exists(p) for p in inputs)
    assert os.path.basename(hip_build.FORMATS_OUT) == "libcroformats.so"
    # the other libraries' lists have not learned the new files
    others = (hip_build.ALL_SRCS + hip_build.ALL_HEADERS + hip_build.SCRUB_HEADERS
              + hip_build.LDS_SCRUB_HEADERS + hip_build.REG_SCRUB_HEADERS)
    assert not {"formats.hip", "croformats.h"} & {os.path.basename(p) for p in others}
    files = {}
    for name in ("formats.hip", "croformats.h", "crohost.h", "cromfma.h", "crocoverage.h",
                 "probe.hip", "croprobe.h", "croagent.cpp"):
        files[name] = tmp_path / name
        files[name].write_text("")
        os.utime(files[name], (100, 100))
    out = tmp_path / "libcroformats.so"
    monkeypatch.setattr(hip_build, "FORMATS_SRC", str(files["formats.hip"]))
    monkeypatch.setattr(hip_build, "FORMATS_HEADERS", [
        str(files[n]) for n in ("croformats.h", "crohost.h", "cromfma.h", "crocoverage.h")])
    monkeypatch.setattr(hip_build, "FORMATS_OUT", str(out))
    commands = []

    def fake_run(argv, check=True):
        commands.append(argv)
        target = argv[argv.index("-o") + 1]
        open(target, "a").close()
        os.utime(target, (400, 400))

    monkeypatch.setattr(hip_build.subprocess, "run", fake_run)
    assert hip_build.build_formats() == str(out)  # missing: built
    assert commands == [[hip_build.HIPCC, *hip_build.DEVICE_FLAGS, "-fPIC", "-shared",
                         str(files["formats.hip"]), "-o", str(out)]]
    commands.clear()
    hip_build.build_formats()
    assert commands == []  # up to date
    for name in ("formats.hip", "croformats.h", "crohost.h", "cromfma.h", "crocoverage.h"):
        os.utime(out, (200, 200))
        os.utime(files[name], (300, 300))
        hip_build.build_formats()
        assert len(commands) == 1, name
        commands.clear()
        os.utime(files[name], (100, 100))
    os.utime(out, (200, 200))
    for name in ("probe.hip", "croprobe.h", "croagent.cpp"):
        os.utime(files[name], (300, 300))  # not its inputs
    hip_build.build_formats()
    assert commands == []
    hip_build.build_formats(force=True)
    assert len(commands) == 1


def test_the_module_and_the_entry_build_the_formats_library_last(monkeypatch, capsys):
    import runpy

    built = []
    for name in ("build", "build_scrub", "build_lds_scrub", "build_reg_scrub", "build_formats"):
        monkeypatch.setattr(hip_build, name,
                            lambda force=False, name=name: built.append((name, force)) or name)
    entry = runpy.run_path(os.path.join(REPO, "__graft_entry__.py"))
    entry["build"]()
    assert built == [("build", True), ("build_scrub", True), ("build_lds_scrub", True),
                     ("build_reg_scrub", True), ("build_formats", True)]
    assert "built build_formats" in capsys.readouterr().out.splitlines()
    with open(hip_build.__file__) as f:
        main_block = f.read().split('if __name__ == "__main__":')[1]
    assert 'print(build_formats(force="--force" in sys.argv))' in main_block
