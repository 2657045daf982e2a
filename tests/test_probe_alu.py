"""CPU tests of the ALU probe stage: the form list, operand rows and references
of croalu.h against their second statement in nodeops/alu.py (bit for bit, from
a host-only program that also runs clean under the address and undefined-
behaviour sanitizers), the struct layouts, the edge rows, the exactness bound
of the fma forms, the aggregation with the digest majority, the stage's
assembly, and the plumbing from the operator's flags to the controller's
message.  Nothing here needs a GPU."""

import argparse
import ctypes
import logging
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cro_amd.api.v1alpha1.types import ComposableResource, Event
from cro_amd.fabric.base import FabricError
from cro_amd.hip import build as hip_build
from cro_amd.nodeops import alu as A
from cro_amd.nodeops import probe as probe_mod
from tests.conftest import make_node, make_resource

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(REPO, "cro_amd", "hip")
AGENT = os.path.join(REPO, "cro_amd", "agent", "croagent")

ALU_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "croalu.h"

int main(int argc, char** argv) {
  if (argc >= 3 && argv[1][0] == 't') {
    const uint32_t seed = (uint32_t)strtoul(argv[2], 0, 0);
    std::vector<uint32_t> w((size_t)CRO_ALU_FORM_COUNT * 64 * 8);
    cro_alu_table(seed, w.data());
    for (int f = 0; f < CRO_ALU_FORM_COUNT; ++f) {
      const CroAluForm* fm = cro_alu_form(f);
      printf("form %d %s %s %s %d %d %d\n", f, kCroAluTestNames[fm->check], fm->name,
             fm->mnemonic, fm->nsrc, fm->nres, cro_alu_checked_rows(fm->check, f));
      for (int r = 0; r < 64; ++r) {
        for (int k = 0; k < 8; ++k) printf("%08x ", w[((size_t)f * 64 + r) * 8 + k]);
        printf("\n");
      }
    }
  } else if (argc >= 2 && argv[1][0] == 'l') {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(CroAluOpts), sizeof(CroAluRecord),
           sizeof(CroAluAgg), sizeof(CroAluResult), offsetof(CroAluResult, agg),
           offsetof(CroAluResult, first_bad_round), offsetof(CroAluResult, msg),
           offsetof(CroAluOpts, min_cu_fraction));
  } else if (argc >= 2 && argv[1][0] == 'a') {
    std::vector<CroAluRecord> recs;
    CroAluRecord r;
    while (scanf("%u %u %u %u %u %u %u %u", &r.xcc_id, &r.hw_id, &r.fail_mask, &r.n_bad,
                 &r.first_bad, &r.bits_bad, &r.valid, &r.digest) == 8)
      recs.push_back(r);
    CroAluAgg a;
    cro_alu_aggregate(recs.data(), recs.size(), &a);
    printf("waves_run %llu\nwaves_bad %llu\n", a.waves_run, a.waves_bad);
    for (int t = 0; t < CRO_ALU_TESTS; ++t) printf("bad_%s %llu\n", kCroAluTestNames[t], a.bad[t]);
    printf("cus_seen %d\nxcds_seen %d\nsimds_seen %d\ncus_bad %d\nxcd %d\nse %d\nsh %d\ncu %d\n"
           "simd %d\nfail_mask %u\nfirst_fail_mask %u\nn_bad %u\nfirst_bad %u\nbits_bad %u\n"
           "first_bad_index %lld\ndigest %u\nno_majority %u\ndigest_waves %llu\n",
           a.cus_seen, a.xcds_seen, a.simds_seen, a.cus_bad, a.xcd, a.se, a.sh, a.cu, a.simd,
           a.fail_mask, a.first_fail_mask, a.n_bad, a.first_bad, a.bits_bad, a.first_bad_index,
           a.digest, a.no_majority, a.digest_waves);
  }
  return 0;
}
"""


def _host_cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    pytest.fail("no host C++ compiler (c++/g++/clang++) on PATH")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def alu_exe(request, tmp_path_factory):
    extra = ()
    if request.param == "sanitized":
        extra = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    tmp = tmp_path_factory.mktemp(f"alu-{request.param}")
    src = tmp / "alu_main.cpp"
    src.write_text(ALU_MAIN)
    exe = tmp / "alu_main"
    subprocess.run([_host_cxx(), "-std=c++17", "-O1", *extra, f"-I{HIP_DIR}", str(src), "-o",
                    str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


def _run(exe, *args, stdin=None):
    out = subprocess.run([exe, *map(str, args)], input=stdin, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout


_tables = {}


def _table(seed):
    """The mirror's table of a seed: computed once, shared, read-only."""
    if seed not in _tables:
        table = A.alu_table(seed)
        table.setflags(write=False)
        _tables[seed] = table
    return _tables[seed]


def _forms_of(*classes):
    return [i for i, f in enumerate(A.alu_forms()) if f[4] in classes]


# -- the header against the mirror ----------------------------------------------------------


@pytest.mark.parametrize("seed", (0, 5))
def test_forms_rows_and_expected_words_match_the_header(alu_exe, seed):
    lines = _run(alu_exe, "t", seed).splitlines()
    forms = A.alu_forms()
    assert len(lines) == 65 * len(forms)
    table = _table(seed)
    for f, fm in enumerate(forms):
        head = lines[65 * f].split()
        assert head == ["form", str(f), A.ALU_TESTS[fm[0]], fm[1], fm[2],
                        *map(str, A.SIGS[fm[3]]), str(A.checked_rows(f))]
        rows = np.array([[int(w, 16) for w in line.split()]
                         for line in lines[65 * f + 1:65 * f + 65]], dtype=np.uint32)
        assert np.array_equal(rows, table[f]), (fm[1], np.argwhere(rows != table[f])[:4])


def test_form_list_shape():
    forms = A.alu_forms()
    names = [f[1] for f in forms]
    assert len(set(names)) == len(names) and len(forms) < 1 << 19  # first_bad holds form << 13
    checks = [f[0] for f in forms]
    assert checks == sorted(checks) and set(checks) == set(range(12))  # fail-mask order
    assert all(f[3] in A.SIGS for f in forms)
    # a few hundred KiB: the table stays in L2
    assert 100 << 10 < len(forms) * 64 * 8 * 4 < 1 << 20


def test_struct_layouts_match_ctypes(alu_exe):
    sizes = [int(x) for x in _run(alu_exe, "l").split()]
    n_agg = sum(ctypes.sizeof(t) for _, t in A.ALU_AGG_FIELDS)
    assert sizes == [
        ctypes.sizeof(A.CroAluOpts), ctypes.sizeof(A.CroAluRecord), n_agg,
        ctypes.sizeof(A.CroAluResult), A.CroAluResult.waves_run.offset,
        A.CroAluResult.first_bad_round.offset, A.CroAluResult.msg.offset,
        A.CroAluOpts.min_cu_fraction.offset,
    ]
    assert ctypes.sizeof(A.CroAluRecord) == 32 and A.CroAluRecord.digest.offset == 28


# -- edge rows and exactness ---------------------------------------------------------------------


def test_integer_edge_rows_are_in_every_integer_form():
    table = _table(0)
    edges = np.array(A.INT_EDGES, dtype=np.uint32)
    forms = _forms_of("INT")
    assert len(forms) > 100
    for f in forms:
        assert np.array_equal(table[f, :len(edges), :6], edges), A.alu_forms()[f][1]
    words = {int(w) for w in edges.reshape(-1)}
    assert {0, 1, 0xFFFFFFFF, 0x80000000, 0xFFFF, 0xFFFFFF, 31, 32, 63} <= words
    # carries out of bits 15, 23 and 31 of s0 + s1; counts 0, 31, 32, 63 first and second
    assert [tuple(e[:2]) for e in A.INT_EDGES[4:7]] == [(0xFFFF, 1), (0xFFFFFF, 1),
                                                          (0xFFFFFFFF, 1)]
    assert [e[0] for e in A.INT_EDGES[7:11]] == [0, 31, 32, 63]
    assert [e[1] for e in A.INT_EDGES[11:15]] == [0, 31, 32, 63]


def test_float_edge_rows_are_in_every_form_of_their_class():
    table = _table(0)
    edges = np.array(A.F32_EDGES, dtype=np.uint32)
    for f in _forms_of("F32"):
        assert np.array_equal(table[f, :len(edges), :3], edges)
    first = {e[0] for e in A.F32_EDGES} | {e[1] for e in A.F32_EDGES}
    # +-0, smallest / largest normal and subnormal
    assert {0, 0x80000000, 0x00800000, 0x7F7FFFFF, 1, 0x007FFFFF} <= first
    add = A.form_index("add_f32")
    # ties to even in both directions and overflow to infinity, as add_f32 sees them
    assert int(table[add, 6, 6]) == 0x3F800000 and int(table[add, 7, 6]) == 0x3F800002
    assert int(table[add, 3, 6]) == 0x7F800000 and int(table[add, 8, 6]) == 0x7F800000
    for f in _forms_of("F64", "F64R"):
        lo_hi = table[f, :len(A.F64_EDGES), :4].astype(np.uint64)
        got = [(int(r[0] | (r[1] << 32)), int(r[2] | (r[3] << 32))) for r in lo_hi]
        assert got == list(A.F64_EDGES)
    # the fma classes of f64 and f16 have edge rows of their own, within their bounds
    f = A.form_index("fma_f64")
    got = [tuple(int(r[2 * k]) | (int(r[2 * k + 1]) << 32) for k in range(3))
           for r in table[f, :len(A.F64FMA_EDGES)]]
    assert got == list(A.F64FMA_EDGES)
    assert {0, 1 << 63, 1, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF} <= {v for e in got for v in e}
    assert (int(table[f, 4, 6]), int(table[f, 4, 7])) == (0, 0x3FF00000)  # the tie rounds down
    assert (int(table[f, 5, 6]), int(table[f, 5, 7])) == (2, 0x3FF00000)  # and up
    assert int(table[f, 6, 7]) == 0x7FF00000  # overflow to infinity
    for g in _forms_of("F16FMA"):
        assert [tuple(int(w) for w in r[:3]) for r in table[g, :len(A.F16FMA_EDGES)]] == \
            list(A.F16FMA_EDGES)
    halves = {h for e in A.F16FMA_EDGES for w in e for h in (w & 0xFFFF, w >> 16)}
    assert {0, 0x8000, 1, 0x03FF, 0x0400, 0x7BFF} <= halves
    pk = A.form_index("pk_fma_f16")
    assert int(table[pk, 4, 6]) >> 16 == 0x7C00 and int(table[pk, 3, 6]) & 0xFFFF == 2
    # no infinity or NaN among the sources outside the forms named for them
    for f, fm in enumerate(A.alu_forms()):
        if fm[4] in ("F32", "F32FMA", "F32PKFMA", "F32H"):
            n = A.SIGS[fm[3]][0]
            assert not np.any((table[f, :, :n] & 0x7F800000) == 0x7F800000), fm[1]


def _e(bits):
    return math.frexp(A.f32(bits))[1] - 1


@pytest.mark.parametrize("seed", (0, 5))
def test_fma_operands_satisfy_the_exactness_bound(seed):
    table = _table(seed)
    triples = {"F32FMA": ((0, 1, 2),), "F32PKFMA": ((0, 2, 4), (1, 3, 5))}
    n = 0
    for f, fm in enumerate(A.alu_forms()):
        for ia, ib, ic in triples.get(fm[4], ()):
            for row in table[f]:
                a, b, c = int(row[ia]), int(row[ib]), int(row[ic])
                if 0 in (a & 0x7FFFFFFF, b & 0x7FFFFFFF, c & 0x7FFFFFFF):
                    continue
                assert A.FMA_LO <= _e(a) + _e(b) - _e(c) <= A.FMA_HI, (fm[1], row)
                n += 1
        if fm[4] == "F16FMA":  # product and addend together span fewer than 53 bits
            for row in table[f]:
                for ha in (row[0] & 0xFFFF, row[0] >> 16):
                    for hb in (row[1] & 0xFFFF, row[1] >> 16):
                        for hc in (row[2] & 0xFFFF, row[2] >> 16):
                            va, vb, vc = A.half(int(ha)), A.half(int(hb)), A.half(int(hc))
                            top = max(math.frexp(va * vb)[1], math.frexp(vc)[1]) + 1
                            low = min(math.frexp(va * vb)[1] - 22, math.frexp(vc)[1] - 11)
                            assert top - low <= 53
    assert n > 200


def test_f64_add_mul_fma_results_are_exact():
    from fractions import Fraction

    table = _table(5)
    for name, fn in (("add_f64", lambda a, b, c: a + b), ("mul_f64", lambda a, b, c: a * b),
                     ("fma_f64", lambda a, b, c: a * b + c)):
        f = A.form_index(name)
        for row in table[f, len(A.F64_EDGES):]:
            a, b, c = (Fraction(A.f64(int(row[2 * i]), int(row[2 * i + 1]))) for i in range(3))
            assert Fraction(A.f64(int(row[6]), int(row[7]))) == fn(a, b, c), name


def test_divide_rows_reach_the_scale_path():
    table = _table(0)
    f = A.form_index("div_f64")
    b = [A.f64(int(r[2]), int(r[3])) for r in table[f]]
    q = [A.f64(int(r[6]), int(r[7])) for r in table[f]]
    assert any(0 < abs(x) < 2.0 ** -1022 for x in b)  # a tiny divisor
    assert any(2.0 ** 900 < abs(x) < math.inf for x in q)  # a huge quotient
    assert not any(x != x for x in q)


def test_transcendental_anchor_rows_are_exact_values():
    table = _table(0)
    for name, fn in (("t_exp_f32", lambda x: 2.0 ** x), ("t_log_f32", math.log2),
                     ("t_rcp_f32", lambda x: 1 / x), ("t_sqrt_f32", math.sqrt)):
        f = A.form_index(name)
        for row in table[f, :A.ANCHORS]:
            x, y = A.f32(int(row[0])), A.f32(int(row[6]))
            assert fn(x) == y and (y == int(y) or 1 / y == int(1 / y)), (name, x, y)
    assert A.checked_rows(A.form_index("t_sqrt_f64")) == 0
    assert A.checked_rows(A.form_index("t_rcp_f64")) == A.ANCHORS
    assert A.checked_rows(A.form_index("mul_lo_u32")) == 64


def test_perm_and_class_rows_cover_every_code():
    table = _table(0)
    sel = table[A.form_index("perm_b32"), :, 2]
    codes = {(int(s) >> (8 * i)) & 255 for s in sel for i in range(4)}
    assert codes == set(range(16))  # all 16 selector codes
    cls = table[A.form_index("cmp_class_f32")]
    assert [int(r[1]) for r in cls[:10]] == [1 << i for i in range(10)]
    assert all(int(r[6]) == 1 for r in cls[:10])  # row i: a value of class i, mask bit i


# -- aggregation ---------------------------------------------------------------------------------


def _records(rows):
    dtype = np.dtype([(n, np.uint32) for n, _ in A.CroAluRecord._fields_])
    return np.array([tuple(r) for r in rows], dtype=dtype)


def _header_aggregate(exe, records):
    text = "\n".join(" ".join(str(int(v)) for v in r) for r in records)
    out = {}
    for line in _run(exe, "a", stdin=text + "\n").splitlines():
        key, value = line.split()
        out[key] = int(value)
    return out


def _hw(se, cu, simd):
    return (se << 13) | (cu << 8) | (simd << 4)


def test_aggregate_lowest_check_leads_and_counts_cus_not_waves(alu_exe):
    d = 0xABCD1234
    rows = [(1, _hw(0, 3, s), 0, 0, 0xFFFFFFFF, 0, 1, d) for s in range(4)]
    rows += [(2, _hw(1, 5, 0), (1 << A.F32) | (1 << A.CMP), 7, A.alu_elem(60, 0, 3, 17), 0x10, 1, d),
             (2, _hw(1, 5, 1), 1 << A.CMP, 2, 9, 0x20, 1, d),
             (2, _hw(1, 6, 1), 1 << A.INT, 1, 5, 0x40, 1, d),
             (0, 0, 0xFF, 9, 9, 9, 0, 77)]  # not valid: ignored
    recs = _records(rows)
    want = A.aggregate_alu_records(recs)
    got = _header_aggregate(alu_exe, recs)
    assert got == want
    assert want["waves_run"] == 7 and want["waves_bad"] == 3
    assert want["cus_seen"] == 3 and want["cus_bad"] == 2 and want["simds_seen"] == 7
    assert want["first_bad_index"] == 4 and want["first_fail_mask"] == (1 << A.F32) | (1 << A.CMP)
    assert A.alu_test_name(want["first_fail_mask"]) == "f32"  # the lowest check leads
    assert want["bad_f32"] == 1 and want["bad_compare_select"] == 2 and want["bad_int_arith"] == 1
    assert want["digest"] == d and want["digest_waves"] == 7 and want["no_majority"] == 0


def test_aggregate_clean_and_empty(alu_exe):
    clean = _records([(0, _hw(0, c, s), 0, 0, 0xFFFFFFFF, 0, 1, 5) for c in range(3)
                      for s in range(4)])
    for recs in (clean, _records([])):
        want = A.aggregate_alu_records(recs)
        assert _header_aggregate(alu_exe, recs) == want
        assert want["waves_bad"] == 0 and want["first_bad_index"] == -1
        assert want["first_bad"] == 0xFFFFFFFF and want["fail_mask"] == 0
        assert (want["xcd"], want["cu"], want["simd"]) == (-1, -1, -1)
    assert A.aggregate_alu_records(clean)["digest"] == 5
    empty = A.aggregate_alu_records(_records([]))
    assert empty["waves_run"] == 0 and empty["digest"] == 0 and empty["no_majority"] == 0


def test_aggregate_consensus_flags_the_deviating_wave(alu_exe):
    rows = [(0, _hw(0, c, s), 0, 0, 0xFFFFFFFF, 0, 1, 0x1111) for c in range(2) for s in range(4)]
    rows[5] = rows[5][:7] + (0x1131,)
    # a wave that failed another check as well keeps that check's element
    rows[6] = (0, _hw(0, 1, 2), 1 << A.BIT, 3, 44, 0x8, 1, 0x9999)
    recs = _records(rows)
    want = A.aggregate_alu_records(recs)
    assert _header_aggregate(alu_exe, recs) == want
    assert want["digest"] == 0x1111 and want["digest_waves"] == 6
    assert want["waves_bad"] == 2 and want["bad_transcendental"] == 2 and want["bad_bit_ops"] == 1
    assert want["first_bad_index"] == 5 and want["first_bad"] == 0xFFFFFFFF
    assert want["bits_bad"] == 0x20 and want["first_fail_mask"] == 1 << A.TRANS
    assert want["cus_bad"] == 1
    assert not recs["fail_mask"][5]  # a private copy: the caller's records are untouched


def test_aggregate_without_a_strict_majority_flags_every_wave(alu_exe):
    rows = [(0, _hw(0, 0, s), 0, 0, 0xFFFFFFFF, 0, 1, 1 + (s & 1)) for s in range(4)]
    recs = _records(rows)
    want = A.aggregate_alu_records(recs)
    assert _header_aggregate(alu_exe, recs) == want
    assert want["no_majority"] == 1 and want["digest"] == 0 and want["digest_waves"] == 0
    assert want["waves_bad"] == 4 and want["bad_transcendental"] == 4 and want["bits_bad"] == 0


def test_every_scalar_form_that_defines_scc_captures_it():
    # 32-bit results carry SCC as their second word; a form whose result fills
    # both words has a twin, <name>_scc, that runs the instruction again and
    # keeps SCC alone
    forms = {f[1]: f for f in A.alu_forms()}
    defines = [f"s_{op}_{w}" for op in ("and", "or", "xor", "nand", "nor", "xnor", "andn2", "orn2")
               for w in ("b32", "b64")]
    defines += ["s_lshl_b32", "s_lshr_b32", "s_ashr_i32", "s_lshl_b64", "s_lshr_b64", "s_ashr_i64",
                "s_bfe_u32", "s_bfe_i32", "s_bfe_u64", "s_bfe_i64", "s_not_b32", "s_bcnt0_i32_b32",
                "s_bcnt1_i32_b64", "s_absdiff_i32", "s_min_i32", "s_max_u32", "s_add_u64",
                "s_sub_u64"] + [f"s_lshl{n}_add_u32" for n in (1, 2, 3, 4)]
    for name in defines:
        sig = forms[name][3]
        assert sig.startswith("S1C") or forms[name + "_scc"][3].startswith("SC_"), name
    table = _table(0)
    for name in ("s_and_b64", "s_lshr_b64", "s_bfe_i64"):
        base, scc = A.form_index(name), table[A.form_index(name + "_scc")]
        # on the twin's own rows: SCC is "the base form's result is not zero"
        want = [int(any(A.alu_reference(base, r[:6]))) for r in scc]
        assert [int(v) for v in scc[:, 6]] == want and 0 < sum(want) < 64
    carry = table[A.form_index("s_add_u64_scc")]
    assert 0 < carry[:, 6].sum() < 64 and int(carry[2, 6]) == 1  # all ones + all ones


def test_describe_first_bad():
    f = A.form_index("mul_hi_u32")
    assert A.describe_first_bad(A.alu_elem(f, 0, 3, 17)) == "form v_mul_hi_u32 row 3 lane 17"
    assert A.decode_first_bad(A.alu_elem(f, 1, 63, 62)) == {"form": f, "word": 1, "row": 63,
                                                             "lane": 62}
    assert A.describe_first_bad(0xFFFFFFFF) == "digest differs"


# -- the stage's assembly --------------------------------------------------------------------------


@pytest.fixture(scope="module")
def stage_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("alu-asm") / "alu.s"
    subprocess.run([hip_build.HIPCC, *hip_build.DEVICE_FLAGS, "-S", "--cuda-device-only",
                    hip_build.ALU_SRC, "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    start = text.index("alu_kernel")
    kernel = text[start:text.index("s_endpgm", start)]
    return text, kernel


def test_stage_kernel_holds_every_mnemonic_of_the_form_list(stage_asm):
    _, kernel = stage_asm
    for _, name, mnemonic, *_ in A.alu_forms():
        assert re.search(rf"\b{mnemonic}(_e32|_e64|_sdwa)?\b", kernel), name
    for op in ("v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64", "v_rcp_f64", "v_rsq_f64",
               "v_readfirstlane_b32", "v_cndmask_b32", "s_cselect_b32"):
        assert op in kernel, op
    for modifier in ("op_sel:[1,0]", "op_sel_hi:[0,1]", "dst_unused:UNUSED_PRESERVE",
                     "sext(", "clamp", "bitop3:0x96", "bitop3:0xe8"):
        assert modifier in kernel, modifier


def test_stage_kernel_keeps_denormals_and_uses_no_scratch(stage_asm):
    text, _ = stage_asm
    m = re.search(r"\.amdhsa_kernel \S*alu_kernel\S*\n(.*?)\.end_amdhsa_kernel", text, re.S)
    desc = m.group(1)
    # hipcc's default kernel mode: f32 and f16 / f64 denormals on (3 = in and out)
    assert ".amdhsa_float_denorm_mode_32 3" in desc
    assert ".amdhsa_float_denorm_mode_16_64 3" in desc
    assert ".amdhsa_ieee_mode 1" in desc
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc)
    assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 256  # the architected VGPRs of a wave


# -- staging ------------------------------------------------------------------------------------------


class Gpu:
    pci_bdf = "0000:05:00.0"


GOOD_QUICK = {"ok": True, "rc": 0, "mfma_f32_exact": True, "hbm_gbps": 4000.0, "msg": "ok"}
GOOD_STAGE = {
    "ok": True, "rc": 0, "cus_expected": 256, "cus_seen": 256, "xcds_seen": 8,
    "simds_seen": 1024, "rounds": 1, "waves_run": 1024, "waves_bad": 0, "cus_bad": 0,
    "failed_test": "", "gpu_ms": 0.134, "msg": "ok",
}
GOOD_ALU = dict(GOOD_STAGE, gpu_ms=0.16, first_bad=0xFFFFFFFF, digest=0x1234)
BAD_ALU = dict(GOOD_ALU, ok=False, rc=-38, failed_test="int_arith", xcd=5, se=2, sh=0, cu=7,
               simd=3, waves_bad=4, cus_bad=1, first_bad=A.alu_elem(3, 0, 9, 17),
               bits_bad=0x00010000, msg="alu mismatch in int_arith")
GOOD_INTEGRITY = {
    "ok": True, "rc": 0, "n_bad": 0, "failed_stage": "", "msg": "ok",
    "vram_passes": 2, "vram_bytes_verified": 2 << 30,
    "h2d_dma_bytes_verified": 256 << 20, "d2h_dma_bytes_verified": 256 << 20,
    "h2d_dma_gbps": 51.5, "d2h_dma_gbps": 49.0,
}


def _patch_probe(monkeypatch, alu=GOOD_ALU, movement=GOOD_STAGE, integrity=GOOD_INTEGRITY):
    from cro_amd.nodeops import coherence as C
    from cro_amd.nodeops import formats as F
    from cro_amd.nodeops import movement as M

    order = []

    def runner(name, result):
        def run(device=0, **kw):
            order.append((name, device, kw))
            return dict(result)
        return run

    monkeypatch.setattr(probe_mod, "hip_device_for_bdf", lambda bdf: 3)
    monkeypatch.setattr(probe_mod, "run_probe", runner("quick", GOOD_QUICK))
    monkeypatch.setattr(probe_mod, "run_compute", runner("compute", GOOD_STAGE))
    monkeypatch.setattr(F, "run_formats", runner("formats", GOOD_STAGE))
    monkeypatch.setattr(C, "run_coherence", runner("coherence", GOOD_STAGE))
    monkeypatch.setattr(M, "run_movement", runner("movement", movement))
    monkeypatch.setattr(A, "run_alu", runner("alu", alu))
    monkeypatch.setattr(probe_mod, "run_integrity", runner("integrity", integrity))
    return order


def _stages(order):
    return [name for name, _, _ in order]


def test_alu_off_returns_todays_hooks(monkeypatch):
    assert probe_mod.make_probe_fn("quick", alu=False) is probe_mod.probe_fn_for_nodeops
    order = _patch_probe(monkeypatch)
    fn = probe_mod.make_probe_fn("deep", compute=True, movement=True, alu=False)
    assert fn(Gpu()) == dict(GOOD_QUICK, compute=GOOD_STAGE, movement=GOOD_STAGE,
                             integrity=GOOD_INTEGRITY)
    assert _stages(order) == ["quick", "compute", "movement", "integrity"]
    assert not hasattr(fn, "alu")


def test_stage_order_and_result(monkeypatch):
    order = _patch_probe(monkeypatch)
    fn = probe_mod.make_probe_fn("deep", compute=True, formats=True, coherence=True,
                                 movement=True, alu=True, seed=9, alu_min_cu_fraction=0.5)
    result = fn(Gpu())
    assert _stages(order) == ["quick", "compute", "formats", "coherence", "movement", "alu",
                              "integrity"]
    assert order[5][1] == 3 and order[5][2] == {"seed": 9, "min_cu_fraction": 0.5}
    assert list(result)[-3:] == ["movement", "alu", "integrity"] and result["ok"] is True
    order.clear()
    quick = probe_mod.make_probe_fn("quick", alu=True)
    assert quick(Gpu()) == dict(GOOD_QUICK, alu=GOOD_ALU) and quick.alu is True
    assert _stages(order) == ["quick", "alu"]


def test_stops_at_the_first_failing_stage(monkeypatch):
    fn = probe_mod.make_probe_fn("deep", movement=True, alu=True)
    order = _patch_probe(monkeypatch, movement=dict(GOOD_STAGE, ok=False, msg="m"))
    result = fn(Gpu())
    assert _stages(order) == ["quick", "movement"] and "alu" not in result
    order = _patch_probe(monkeypatch, alu=BAD_ALU)
    result = fn(Gpu())
    assert _stages(order) == ["quick", "movement", "alu"]
    assert result["ok"] is False and result["msg"] == BAD_ALU["msg"]
    assert result["alu"] == BAD_ALU and "integrity" not in result


def test_run_alu_builds_its_options(monkeypatch):
    seen = {}

    class Lib:
        @staticmethod
        def cro_alu_run(device, opts, res):
            o = ctypes.cast(opts, ctypes.POINTER(A.CroAluOpts)).contents
            seen.update({name: getattr(o, name) for name, _ in A.CroAluOpts._fields_})
            seen["device"] = device
            return -39

    monkeypatch.setattr(A, "load_alu_library", lambda required=None: Lib)
    elem = A.alu_elem(A.form_index("mul_f32"), 0, 5, 5)
    out = A.run_alu(2, grid_blocks=3, iters=5, max_rounds=2, seed=-1, min_cu_fraction=0.25,
                    selftest_mode=1, selftest_test="f32", selftest_bit=30, selftest_elem=elem,
                    selftest_key=0x50700, selftest_also="add_u64")
    assert seen == {"device": 2, "grid_blocks": 3, "iters": 5, "max_rounds": 2,
                    "seed": 0xFFFFFFFF, "selftest_mode": 1, "selftest_test": A.F32,
                    "selftest_bit": 30, "selftest_elem": elem, "selftest_key": 0x50700,
                    "selftest_also": 1, "min_cu_fraction": 0.25}
    assert out["ok"] is False and out["rc"] == -39 and list(out)[:2] == ["ok", "rc"]
    assert [k for k in out if k.startswith("bad_")] == [f"bad_{n}" for n in A.ALU_TESTS]
    assert {"digest", "digest_waves", "no_majority", "failed_test", "msg"} <= set(out)
    with pytest.raises(TypeError):
        A.run_alu(0, lds_bytes=1)


def test_loader_without_the_library(monkeypatch, tmp_path):
    monkeypatch.setattr(A, "_lib", None)
    monkeypatch.setattr(A, "_LIB_PATH", str(tmp_path / "libcroalu.so"))
    assert A.load_alu_library(required=False) is None
    with pytest.raises(RuntimeError, match="libcroalu.so missing"):
        A.load_alu_library(required=True)
    with pytest.raises(RuntimeError):
        A.run_alu(0)  # never a silent pass
    with pytest.raises(RuntimeError):
        A.alu_tile(0, "add_f32", np.zeros((64, 6), dtype=np.uint32))


class RecordingExec:
    def __init__(self, stdout):
        self.stdout, self.argvs = stdout, []

    def run(self, node, argv, timeout=0):
        self.argvs.append(list(argv))
        return 0, self.stdout, ""


def test_exec_probe_argv_with_and_without_alu():
    ex = RecordingExec('{"ok": true, "alu": {"ok": true}}')
    base = ["croagent", "probe", "--bdf", "0000:05:00.0"]
    probe_mod.probe_via_exec(ex, "n0", Gpu())
    probe_mod.probe_via_exec(ex, "n0", Gpu(), alu=False, alu_min_cu_fraction=0.9)
    assert probe_mod.probe_via_exec(ex, "n0", Gpu(), alu=True)["alu"]["ok"] is True
    probe_mod.probe_via_exec(ex, "n0", Gpu(), level="deep", vram_mib=64, movement=True, alu=True,
                             alu_min_cu_fraction=0.9)
    probe_mod.make_exec_probe_fn(ex, "n0", alu=True, alu_min_cu_fraction=1)(Gpu())
    assert ex.argvs == [
        base, base, base + ["--alu"],
        base + ["--deep", "--vram-mib", "64", "--movement", "--alu", "--alu-min-cu-fraction",
                "0.9"],
        base + ["--alu", "--alu-min-cu-fraction", "1.0"],
    ]
    assert probe_mod._alu_argv(False, 0.5) == []


def test_a_stage_that_is_off_passes_no_keyword_of_its_own(monkeypatch):
    seen = []
    monkeypatch.setattr(probe_mod, "probe_via_exec",
                        lambda execer, node, gpu, **kw: seen.append(sorted(kw)) or {})
    probe_mod.make_exec_probe_fn(None, "n0")(Gpu())
    probe_mod.make_exec_probe_fn(None, "n0", alu=True)(Gpu())
    today = ["argv_prefix", "compute", "compute_min_cu_fraction", "level", "link_floor_gbps",
             "link_mib", "vram_mib"]
    assert seen == [today, sorted(today + ["alu", "alu_min_cu_fraction"])]


# -- controller ----------------------------------------------------------------------------------------


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


def test_controller_names_check_form_row_lane_and_place(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, ok=False, movement=GOOD_STAGE, alu=BAD_ALU))
    counter = mock_world.resource_rec.metrics.probe_alu_failures_total.labels(test="int_arith")
    before = counter._value.get()
    with pytest.raises(FabricError):
        mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Attaching"
    assert got.status.error.startswith(
        "gfx950 health probe failed: alu stage int_arith form v_mul_hi_u32 row 9 lane 17 "
        "xcd=5 se=2 cu=7 simd=3 bits_bad=0x00010000 cus_bad=1: "), got.status.error
    assert counter._value.get() == before + 1


def test_controller_counts_the_coverage_floor(mock_world):
    floor = dict(GOOD_ALU, ok=False, rc=-39, msg="coverage 3 of 256 CUs")
    _attach(mock_world, dict(GOOD_QUICK, ok=False, alu=floor))
    counter = mock_world.resource_rec.metrics.probe_alu_failures_total.labels(test="coverage")
    before = counter._value.get()
    with pytest.raises(FabricError):
        mock_world.resource_rec.reconcile("gpu-1")
    assert counter._value.get() == before + 1
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.error.startswith(
        "gfx950 health probe failed: alu stage coverage xcd=None"), got.status.error


def test_controller_online_event_carries_the_alu_clause(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, movement=GOOD_STAGE, alu=GOOD_ALU,
                             integrity=GOOD_INTEGRITY))
    mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Online"
    assert _online_message(mock_world) == (
        f"device {got.status.device_id} online with CDI spec"
        "; probe: mfma_exact=True hbm=4000 GB/s"
        "; movement: 256/256 CUs, 1024 SIMDs, 0.1 ms"
        "; alu: 256/256 CUs, 1024 SIMDs, 0.2 ms"
        "; integrity: vram 1.00 GiB link 0.25 GiB verified, h2d 51.5 d2h 49.0 GB/s"
    )


def test_controller_messages_unchanged_without_an_alu_object(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, movement=GOOD_STAGE))
    mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert _online_message(mock_world) == (
        f"device {got.status.device_id} online with CDI spec"
        "; probe: mfma_exact=True hbm=4000 GB/s"
        "; movement: 256/256 CUs, 1024 SIMDs, 0.1 ms"
    )


def test_metrics_reset_unregisters_the_alu_counter():
    from prometheus_client import REGISTRY

    from cro_amd.metrics import Metrics

    Metrics()
    assert "cro_probe_alu_failures" in REGISTRY._names_to_collectors
    Metrics._reset_for_tests()
    try:
        assert "cro_probe_alu_failures" not in REGISTRY._names_to_collectors
    finally:
        Metrics()  # later tests share the process-wide singleton


# -- operator flags ---------------------------------------------------------------------------------------


def _parse(argv):
    from cro_amd.cmd.main import add_probe_arguments

    p = argparse.ArgumentParser()
    add_probe_arguments(p)
    return p.parse_args(argv)


def _clear_env(monkeypatch):
    for stage in ("COMPUTE", "FORMATS", "COHERENCE", "MOVEMENT", "ALU"):
        monkeypatch.delenv(f"CRO_PROBE_{stage}", raising=False)
        monkeypatch.delenv(f"CRO_PROBE_{stage}_MIN_CU_FRACTION", raising=False)
    monkeypatch.delenv("CRO_PROBE_LEVEL", raising=False)


def test_entrypoint_alu_default_off_passes_todays_keywords(monkeypatch):
    from cro_amd.cmd import main as main_mod

    _clear_env(monkeypatch)
    args = _parse([])
    assert args.probe_alu == "off" and args.probe_alu_min_cu_fraction == 0
    assert main_mod.select_probe_fn(args) is probe_mod.probe_fn_for_nodeops
    seen = {}
    monkeypatch.setattr(probe_mod, "make_probe_fn", lambda level, **kw: seen.update(kw))
    main_mod.select_probe_fn(_parse(["--probe-movement", "on"]))
    assert sorted(seen) == ["compute", "compute_min_cu_fraction", "link_bytes", "link_floor_gbps",
                            "movement", "movement_min_cu_fraction", "vram_bytes"]


def test_entrypoint_flag_and_env_select_alu(monkeypatch):
    from cro_amd.cmd.main import select_probe_fn

    _clear_env(monkeypatch)
    fn = select_probe_fn(_parse(["--probe-alu", "on", "--probe-alu-min-cu-fraction", "0.75"]))
    assert fn.level == "quick" and fn.alu is True and fn.compute is False
    order = _patch_probe(monkeypatch)
    assert fn(Gpu())["alu"] == GOOD_ALU and _stages(order) == ["quick", "alu"]
    assert order[1][2]["min_cu_fraction"] == 0.75
    with pytest.raises(SystemExit):
        _parse(["--probe-alu", "maybe"])
    monkeypatch.setenv("CRO_PROBE_ALU", "on")
    monkeypatch.setenv("CRO_PROBE_ALU_MIN_CU_FRACTION", "0.5")
    args = _parse([])
    assert args.probe_alu == "on" and args.probe_alu_min_cu_fraction == 0.5
    assert select_probe_fn(args).alu is True
    # the flag wins over the environment
    assert select_probe_fn(_parse(["--probe-alu", "off"])) is probe_mod.probe_fn_for_nodeops


def test_a_missing_library_warns_and_switches_the_stage_off(monkeypatch, caplog):
    from cro_amd.cmd.main import drop_unavailable_probe_stages, select_probe_fn

    _clear_env(monkeypatch)
    log = logging.getLogger("test-alu")
    args = _parse(["--probe-alu", "on"])
    monkeypatch.setattr(A, "load_alu_library", lambda required=None: object())
    with caplog.at_level(logging.INFO, logger="test-alu"):
        assert drop_unavailable_probe_stages(args, log) is False
    assert args.probe_alu == "on" and "ALU stage: on" in caplog.text
    caplog.clear()
    monkeypatch.setattr(A, "load_alu_library", lambda required=None: None)
    with caplog.at_level(logging.INFO, logger="test-alu"):
        assert drop_unavailable_probe_stages(args, log) is True
    assert args.probe_alu == "off"
    assert "ALU probe library unavailable; alu stage disabled" in caplog.text
    assert select_probe_fn(args) is probe_mod.probe_fn_for_nodeops


# -- native agent and build -----------------------------------------------------------------------------


@pytest.fixture(scope="module")
def agent():
    if not os.path.exists(AGENT) or not os.path.exists(hip_build.OUT):
        hip_build.build()
    return AGENT


def test_croagent_probe_alu_without_a_gpu_leaves_no_trace(agent):
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present: the GPU tests run the stage itself")
    import json

    run = subprocess.run([agent, "probe", "--alu", "--alu-min-cu-fraction", "0.5"],
                         capture_output=True, text=True, timeout=60)
    out = json.loads(run.stdout)
    assert run.returncode == 1 and out["ok"] is False and "alu" not in out, out
    plain = subprocess.run([agent, "probe"], capture_output=True, text=True, timeout=60)
    assert plain.stdout == run.stdout  # a stage that did not run leaves no trace


def test_build_alu_inputs_staleness_and_command(tmp_path, monkeypatch):
    assert hip_build.ALU_SRC == os.path.join(HIP_DIR, "alu.hip")
    assert hip_build.ALU_HEADERS == [os.path.join(HIP_DIR, n) for n in (
        "croalu.h", "crohost.h", "croformats.h", "crocoverage.h")]
    assert hip_build.ALU_OUT == os.path.join(HIP_DIR, "libcroalu.so")
    out = tmp_path / "libcroalu.so"
    monkeypatch.setattr(hip_build, "ALU_OUT", str(out))
    commands = []

    def fake_run(cmd, check=True):
        commands.append(cmd)
        out.write_text("built")

    monkeypatch.setattr(hip_build.subprocess, "run", fake_run)
    assert hip_build.build_alu() == str(out)  # missing: built
    assert commands == [[hip_build.HIPCC, *hip_build.DEVICE_FLAGS, "-fPIC", "-shared",
                         hip_build.ALU_SRC, "-o", str(out)]]
    future = max(os.path.getmtime(p) for p in [hip_build.ALU_SRC] + hip_build.ALU_HEADERS) + 10
    os.utime(out, (future, future))
    hip_build.build_alu()  # fresh: not built again
    assert len(commands) == 1
    hip_build.build_alu(force=True)
    assert len(commands) == 2


def test_the_module_and_the_entry_build_the_alu_library():
    with open(os.path.join(HIP_DIR, "build.py")) as fh:
        main_block = fh.read().split('if __name__ == "__main__":')[1]
    lines = [line.strip() for line in main_block.splitlines() if "print(build_" in line]
    i = lines.index('print(build_alu(force="--force" in sys.argv))')
    assert "build_movement" in lines[i - 1] and "build_reg_scrub" in lines[i + 1]
    with open(os.path.join(REPO, "__graft_entry__.py")) as fh:
        entry = fh.read()
    assert entry.index("build_movement(force=True)") < entry.index("build_alu(force=True)")


def test_docs_name_what_is_not_covered_and_the_profile():
    with open(os.path.join(REPO, "docs", "architecture.md")) as fh:
        doc = fh.read()
    section = doc[doc.index("ALU stage"):]
    assert "Not covered" in section and "common to all SIMDs" in section
    with open(os.path.join(REPO, "profiles", "README.md")) as fh:
        assert "alu_probe_mi355x.md" in fh.read()
