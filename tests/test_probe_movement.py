"""CPU tests of the data-movement probe stage: every check's and variant's
source map, the payload hash, the LDS and global images and the aggregation
of cromovement.h against their numpy mirrors (through a small host program
built with the host C++ compiler, also under the address and
undefined-behaviour sanitizers: no HIP, no GPU), brute-force properties of
the mirrors, the C structs against their ctypes mirrors, the instructions of
the stage's assembly, and the plumbing from the operator flags down to the
agent."""

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
from cro_amd.nodeops import movement as M
from cro_amd.nodeops import probe as probe_mod
from tests.conftest import make_node, make_resource

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(REPO, "cro_amd", "hip")
AGENT = os.path.join(REPO, "cro_amd", "agent", "croagent")
SEEDS = (0, 5, 0xDEADBEEF)
REPS = (0, 1, 63, 64)
TR_CHECKS = (M.TR16, M.TR8, M.TR4, M.TR6)


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
        [_host_cxx(), "-std=c++17", "-O1", *extra, f"-I{HIP_DIR}", str(src), "-o", str(exe)],
        check=True, capture_output=True, text=True,
    )
    return str(exe)


# -- the header against the numpy mirrors -------------------------------------------------

MOVEMENT_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "cromovement.h"

static void maps(uint32_t seed, uint32_t rep) {
  const CroMovRt rt = cro_mov_rt(seed, rep);
  printf("rt %u %u %u %u %u %u\n", rt.salt, rt.sel, rt.fa, rt.wl, rt.a, rt.b);
  for (int t = 0; t < CRO_MOV_TESTS; ++t)
    for (int v = 0; v < cro_mov_variants(t); ++v) {
      printf("regs %d %d %d\n", t, v, cro_mov_regs(t, v));
      if (t <= CRO_MOV_READLANE) {
        for (int r = 0; r < cro_mov_regs(t, v); ++r) {
          printf("src %d %d %d", t, v, r);
          for (int l = 0; l < 64; ++l) printf(" %d", cro_mov_src(t, v, r, l, &rt));
          printf("\n");
        }
        if (t == CRO_MOV_BPERMUTE) {
          printf("idx %d %d 0", t, v);
          for (int l = 0; l < 64; ++l) printf(" %u", cro_mov_bperm_idx(v, (uint32_t)l, &rt));
          printf("\n");
        }
      } else if (t <= CRO_MOV_TR6) {
        printf("addr %d %d 0", t, v);
        for (int l = 0; l < 64; ++l) printf(" %d", cro_mov_tr_addr(t, v, l));
        printf("\nimage %d %d 0", t, v);
        for (int w = 0; w < cro_mov_tr_image_bytes(t, v) / 4; ++w)
          printf(" %u", cro_mov_tr_image_word(t, v, w, rt.salt));
        printf("\n");
      } else {
        printf("addr %d %d 0", t, v);
        for (int l = 0; l < 64; ++l) printf(" %u", cro_mov_dma_addr(v, 3, l, &rt));
        printf("\n");
      }
      for (int r = 0; r < cro_mov_regs(t, v); ++r) {
        printf("want %d %d %d", t, v, r);
        for (int l = 0; l < 64; ++l)
          printf(" %u", t <= CRO_MOV_READLANE ? cro_mov_want(t, v, r, l, &rt)
                        : t <= CRO_MOV_TR6    ? cro_mov_tr_want(t, v, r, l, rt.salt)
                                              : cro_mov_dma_want(v, r, 3, l, &rt));
        printf("\n");
      }
    }
  printf("payload");
  for (int l = 0; l < 64; l += 21) printf(" %u", cro_mov_payload(rt.salt, 3, 1, l, 1));
  printf("\ndma_words %u %u %u\n", cro_mov_dma_word(0), cro_mov_dma_word(1), cro_mov_dma_word(2047));
}

static void layout() {
  printf("{\"opts\":%zu,\"opts.seed\":%zu,\"opts.selftest_also\":%zu,\"opts.min_cu_fraction\":%zu,"
         "\"record\":%zu,\"result\":%zu,\"result.agg\":%zu,\"agg\":%zu,\"agg.bad\":%zu,"
         "\"agg.cus_seen\":%zu,\"agg.fail_mask\":%zu,\"agg.first_bad_index\":%zu,"
         "\"result.first_bad_round\":%zu,\"result.gpu_ms\":%zu,\"result.failed_test\":%zu,"
         "\"result.msg\":%zu}\n",
         sizeof(CroMovementOpts), offsetof(CroMovementOpts, seed),
         offsetof(CroMovementOpts, selftest_also), offsetof(CroMovementOpts, min_cu_fraction),
         sizeof(CroMovementRecord), sizeof(CroMovementResult), offsetof(CroMovementResult, agg),
         sizeof(CroMovementAgg), offsetof(CroMovementAgg, bad), offsetof(CroMovementAgg, cus_seen),
         offsetof(CroMovementAgg, fail_mask), offsetof(CroMovementAgg, first_bad_index),
         offsetof(CroMovementResult, first_bad_round), offsetof(CroMovementResult, gpu_ms),
         offsetof(CroMovementResult, failed_test), offsetof(CroMovementResult, msg));
}

static void aggregate() {
  std::vector<CroMovementRecord> records;
  CroMovementRecord r;
  while (scanf("%u %u %u %u %u %u %u", &r.xcc_id, &r.hw_id, &r.fail_mask, &r.n_bad, &r.first_bad,
               &r.bits_bad, &r.valid) == 7) {
    r.reserved = 0;
    records.push_back(r);
  }
  CroMovementAgg a;
  cro_movement_aggregate(records.data(), records.size(), &a);
  printf("{\"waves_run\":%llu,\"waves_bad\":%llu,", a.waves_run, a.waves_bad);
  for (int t = 0; t < CRO_MOV_TESTS; ++t) printf("\"bad_%s\":%llu,", kCroMovTestNames[t], a.bad[t]);
  printf("\"cus_seen\":%d,\"xcds_seen\":%d,\"simds_seen\":%d,\"cus_bad\":%d,\"xcd\":%d,\"se\":%d,"
         "\"sh\":%d,\"cu\":%d,\"simd\":%d,\"fail_mask\":%u,\"first_fail_mask\":%u,\"n_bad\":%u,"
         "\"first_bad\":%u,\"bits_bad\":%u,\"first_bad_index\":%lld,\"name\":\"%s\"}\n",
         a.cus_seen, a.xcds_seen, a.simds_seen, a.cus_bad, a.xcd, a.se, a.sh, a.cu, a.simd,
         a.fail_mask, a.first_fail_mask, a.n_bad, a.first_bad, a.bits_bad, a.first_bad_index,
         cro_mov_test_name(a.first_fail_mask));
}

int main(int argc, char** argv) {
  if (argc >= 4 && argv[1][0] == 'm') maps((uint32_t)strtoul(argv[2], 0, 0), (uint32_t)atoi(argv[3]));
  else if (argc >= 2 && argv[1][0] == 'l') layout();
  else if (argc >= 2 && argv[1][0] == 'a') aggregate();
  else return 2;
  return 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def movement_exe(request, tmp_path_factory):
    extra = ()
    if request.param == "sanitized":
        extra = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    return _build(tmp_path_factory.mktemp(f"movement-{request.param}"), "movement_main",
                  MOVEMENT_MAIN, extra)


def _run(exe, *args, stdin=None):
    out = subprocess.run([exe, *map(str, args)], input=stdin, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("rep", REPS)
def test_maps_payloads_images_and_addresses_match_the_header(movement_exe, seed, rep):
    lines = _run(movement_exe, "maps", seed, rep).splitlines()
    rt = M.movement_rt(seed, rep)
    assert lines[0].split() == ["rt"] + [str(rt[k]) for k in ("salt", "sel", "fa", "wl", "a", "b")]
    seen = set()
    for line in lines[1:]:
        kind, *rest = line.split()
        if kind == "payload":
            want = M.movement_payload(rt["salt"], 3, 1, np.arange(0, 64, 21), 1)
            assert [int(x) for x in rest] == want.tolist()
            continue
        if kind == "dma_words":
            assert [int(x) for x in rest] == M.dma_source_words()[[0, 1, 2047]].tolist()
            continue
        t, v, r = (int(x) for x in rest[:3])
        values = np.array([int(x) for x in rest[3:]], dtype=np.int64)
        seen.add((kind, t, v))
        if kind == "regs":
            assert r == M.movement_regs(t, v)
        elif kind == "src":
            assert values.tolist() == M.movement_source_map(t, v, rt)[r].tolist(), line
        elif kind == "idx":
            assert values.tolist() == M.bperm_index(v, rt).tolist()
        elif kind == "addr" and t == M.DMA:
            assert values.tolist() == M.dma_addr(v, 3, rt).tolist()
        elif kind == "addr":
            assert values.tolist() == M.tr_addr(t, v).tolist()
        elif kind == "image":
            assert values.tolist() == M.tr_image(t, v, rt["salt"]).tolist()
        else:
            assert kind == "want"
            assert values.tolist() == M.movement_expected(t, v, seed, rep, wave=3)[r].tolist(), line
    for t in range(len(M.MOVEMENT_TESTS)):
        for v in range(M.movement_variants(t)):
            assert ("want", t, v) in seen and ("regs", t, v) in seen


def test_struct_layouts_match_ctypes(movement_exe):
    lay = json.loads(_run(movement_exe, "layout"))
    O, R = M.CroMovementOpts, M.CroMovementResult
    assert lay["opts"] == ctypes.sizeof(O) and lay["opts.seed"] == O.seed.offset
    assert lay["opts.selftest_also"] == O.selftest_also.offset
    assert lay["opts.min_cu_fraction"] == O.min_cu_fraction.offset
    assert lay["record"] == ctypes.sizeof(M.CroMovementRecord) == 32
    assert lay["result"] == ctypes.sizeof(R)
    agg = R.waves_run.offset
    assert lay["result.agg"] == agg
    assert lay["agg.bad"] == R.bad_dpp.offset - agg
    assert R.bad_lds_dma.offset - R.bad_dpp.offset == 8 * 9
    assert lay["agg.cus_seen"] == R.cus_seen.offset - agg
    assert lay["agg.fail_mask"] == R.fail_mask.offset - agg
    assert lay["agg.first_bad_index"] == R.first_bad_index.offset - agg
    assert lay["agg"] == R.first_bad_round.offset - agg
    assert lay["result.first_bad_round"] == R.first_bad_round.offset
    assert lay["result.gpu_ms"] == R.gpu_ms.offset
    assert lay["result.failed_test"] == R.failed_test.offset
    assert lay["result.msg"] == R.msg.offset


# -- properties of the mirrors, by brute force ---------------------------------------------------


@pytest.mark.parametrize("seed", SEEDS)
def test_every_variant_declared_a_permutation_is_a_bijection(seed):
    for rep in REPS:
        rt = M.movement_rt(seed, rep)
        assert rt["a"] % 2 == 1 and rt["a"] not in (1, 63) and 1 <= rt["fa"] <= 63
        assert (rt["a"] * M.inv64(rt["a"])) % 64 == 1
        for t, v in M.PERMUTATIONS:
            codes = M.movement_source_map(t, v, rt)[0]
            assert sorted(codes.tolist()) == list(range(64)), (t, v)
            assert codes.tolist() != list(range(64)), (t, v)  # and not the identity
        # push and pull through the same permutation are inverses
        pull, push = (M.movement_source_map(M.BPERMUTE, v, rt)[0] for v in (0, 2))
        assert pull[push].tolist() == list(range(64))
        # the scatter model of the push agrees with its source map
        src = np.arange(100, 164, dtype=np.uint32)
        assert M.bperm_apply(2, M.bperm_index(2, rt), src).tolist() == src[push].tolist()
        # the many-to-one map really collapses lanes
        assert np.unique(M.movement_source_map(M.BPERMUTE, 1, rt)).size == 32
        # the two swaps move every word exactly once between their two results
        for v in (0, 1):
            both = M.movement_source_map(M.PLSWAP, v, rt)
            assert sorted(both.reshape(-1).tolist()) == list(range(128))
    sels = {M.movement_rt(seed, rep)["sel"] for rep in range(64)}
    assert sels == set(range(64))  # the readlane select sweeps every lane


def test_source_words_of_a_wave_are_distinct():
    rt = M.movement_rt(5, 2)
    lane, reg = np.meshgrid(np.arange(64), np.arange(2))
    words = [M.movement_payload(rt["salt"], t, v, lane, reg).reshape(-1)
             for t in range(5) for v in range(M.movement_variants(t))]
    assert np.unique(np.concatenate(words)).size == sum(w.size for w in words)


def test_dpp_lanes_that_keep_old_are_those_the_masks_and_bound_ctrl_say():
    for v in range(M.movement_variants(M.DPP)):
        codes = M.dpp_source(v)
        keeps = codes >= M.OLD
        assert keeps.tolist() == M.dpp_keeps_old(v).tolist(), v
        assert (codes[keeps] == (M.OLD | np.arange(64))[keeps]).all()  # its own lane's `old`
    zero = {v: np.flatnonzero(M.dpp_source(v) == M.SRC_ZERO).tolist() for v in range(13)}
    assert zero[1] == [15, 31, 47, 63] and zero[7] == [0]
    assert all(not lanes for v, lanes in zero.items() if v not in (1, 7))
    assert np.flatnonzero(M.dpp_keeps_old(2)).tolist() == [0, 1, 2, 16, 17, 18, 32, 33, 34, 48, 49, 50]
    assert np.flatnonzero(M.dpp_keeps_old(6)).tolist() == [63]
    assert np.flatnonzero(M.dpp_keeps_old(10)).tolist() == list(range(16)) + list(range(32, 48))
    assert np.flatnonzero(M.dpp_keeps_old(11)).tolist() == list(range(32))
    # bank_mask 0x5: banks 1 and 3 are masked, and lane 0 of each row has no source
    want = sorted(set(l for l in range(64) if ((l & 15) >> 2) in (1, 3)) | {0, 16, 32, 48})
    assert np.flatnonzero(M.dpp_keeps_old(12)).tolist() == want
    assert M.dpp_source(10)[16:32].tolist() == [15] * 16 and M.dpp_source(11)[32:].tolist() == [31] * 32


@pytest.mark.parametrize("t", TR_CHECKS)
def test_transposed_read_maps_take_each_element_of_each_block_once(t):
    bits, rows, per, nbytes = M.TR_TABLE[t]
    fields = nbytes * 8 // bits
    assert fields == rows and rows * per == 16
    for v in (0, 1):
        stride, addr = M.tr_stride(t, v), M.tr_addr(t, v)
        assert stride % 8 == 0 and (addr % 8 == 0).all()
        image_bytes = 4 * rows * stride
        assert image_bytes <= M.IMAGE_BYTES and (addr + nbytes <= image_bytes).all()
        # label every data field of the image with its own index: the read
        # must deliver every label exactly once, to the lane and field of the map
        label = np.arange(4 * rows * 16).reshape(4, rows, 16)
        got = np.zeros((64, fields), dtype=np.int64)
        for shift in range(0, 10, bits):  # the label, `bits` bits at a time
            piece = (label >> shift) & ((1 << bits) - 1)
            image = np.zeros((4, rows, stride // 4), dtype=np.uint32)
            image[:, :, :16 * bits // 32] = M._pack(piece, bits, 16 * bits // 32)
            regs = M.tr_read(t, image.reshape(-1), addr)
            got |= M._unpack(regs.T.copy(), bits, fields).astype(np.int64) << shift
        assert sorted(got.reshape(-1).tolist()) == list(range(4 * rows * 16))
        lane, q = np.meshgrid(np.arange(64), np.arange(fields), indexing="ij")
        assert (got == label[lane >> 4, q, lane & 15]).all()  # column lane & 15, row q


@pytest.mark.parametrize("t", (M.TR4, M.TR6))
def test_two_pass_codes_tell_every_pair_of_elements_of_a_block_apart(t):
    for salt in (0, 0x2B, 0xFFFFFFFF):
        rows_pass, cols_pass = M.tr_codes(t, 0, salt), M.tr_codes(t, 1, salt)
        for block in range(4):
            pairs = {(int(a), int(b)) for a, b in zip(rows_pass[block].reshape(-1),
                                                       cols_pass[block].reshape(-1))}
            assert len(pairs) == 256
    assert np.unique(M.tr_codes(M.TR16, 0, 77)).size == 256  # distinct over the whole image
    codes8 = M.tr_codes(M.TR8, 0, 77)
    assert all(np.unique(codes8[b]).size == 128 for b in range(4))  # distinct per block


@pytest.mark.parametrize("v", (0, 1, 2))
def test_dma_destination_covers_the_region_once_and_never_the_guard_bands(v):
    n = M.dma_size(v) // 4
    for seed in SEEDS:
        rt = M.movement_rt(seed, 1)
        for wave in range(4):
            addr = M.dma_addr(v, wave, rt)
            assert (addr % M.dma_size(v) == 0).all()
            assert addr.min() >= 0 and addr.max() + M.dma_ioff(v) + M.dma_size(v) <= 4 * M.SRC_WORDS
            chunks = (addr - wave * 1024) // M.dma_size(v)
            assert sorted(chunks.tolist()) == list(range(64))  # a permutation of the wave's chunks
            assert chunks.tolist() != list(range(64))
            # an image that holds its own word index: the region shows where each word came from
            region = M.dma_region(v, np.arange(M.SRC_WORDS, dtype=np.uint32), addr)
            assert (region[:M.GUARD] == M.POISON).all() and (region[-M.GUARD:] == M.POISON).all()
            data = region[M.GUARD:-M.GUARD]
            assert data.size == 64 * n and np.unique(data).size == data.size
            want = ((addr + M.dma_ioff(v)) // 4)[:, None] + np.arange(n)[None, :]
            assert data.tolist() == want.reshape(-1).tolist()
            regs = M.dma_read(v, np.arange(M.SRC_WORDS, dtype=np.uint32), addr)
            assert regs.shape == (M.movement_regs(M.DMA, v), 64)
            assert (regs[n] == M.POISON).all() and regs[:n].reshape(-1).tolist() == data.tolist()
    assert M.POISON not in M.dma_source_words().tolist()


# -- aggregation -----------------------------------------------------------------------------------

FIELDS = ("xcc_id", "hw_id", "fail_mask", "n_bad", "first_bad", "bits_bad", "valid")


def _hw(se, sh, cu, simd, slot=0):
    return (se << 13) | (sh << 12) | (cu << 8) | (simd << 4) | slot


def _both(exe, rows):
    dtype = np.dtype([(name, np.uint32) for name in FIELDS])
    rec = np.array([tuple(r) for r in rows], dtype=dtype)
    text = "\n".join(" ".join(str(x) for x in r) for r in rows) + "\n"
    got = json.loads(_run(exe, "agg", stdin=text))
    name = got.pop("name")
    assert got == M.aggregate_movement_records(rec)
    assert name == M.movement_test_name(got["first_fail_mask"])
    return got, name


def test_aggregate_lowest_check_leads_and_counts_cus_not_waves(movement_exe):
    elem = M.movement_elem(3, 0, 17)
    rows = [
        (1, _hw(2, 0, 5, 0), 0, 0, 0xFFFFFFFF, 0, 1),
        (1, _hw(2, 0, 5, 1), (1 << M.TR8) | (1 << M.SWIZZLE), 2, elem, 0x80000001, 1),
        (1, _hw(2, 0, 5, 2), 1 << M.DPP, 1, 5, 1, 1),       # the same CU again
        (7, _hw(0, 1, 9, 3), 1 << M.DMA, 9, 9, 9, 0),       # invalid: ignored
        (3, _hw(1, 0, 2, 3), 1 << M.TR8, 4, 7, 2, 1),
    ]
    got, name = _both(movement_exe, rows)
    assert got["waves_run"] == 4 and got["waves_bad"] == 3 and got["cus_bad"] == 2
    assert got["cus_seen"] == 2 and got["simds_seen"] == 4 and got["xcds_seen"] == 2
    assert got["fail_mask"] == (1 << M.TR8) | (1 << M.SWIZZLE) | (1 << M.DPP)
    assert got["bad_lds_tr8"] == 2 and got["bad_swizzle"] == 1 and got["bad_dpp"] == 1
    assert got["bad_lds_dma"] == 0
    # the first bad record leads, and of its two checks the lower one names it
    assert got["first_bad_index"] == 1 and name == "swizzle"
    assert (got["xcd"], got["se"], got["sh"], got["cu"], got["simd"]) == (1, 2, 0, 5, 1)
    assert got["first_bad"] == elem and got["bits_bad"] == 0x80000001 and got["n_bad"] == 2
    assert M.decode_first_bad(elem) == {"variant": 3, "register": 0, "lane": 17}
    assert M.describe_first_bad("swizzle", elem) == "variant 3 (broadcast) register 0 lane 17"
    assert M.describe_first_bad("lds_tr6", M.movement_elem(1, 2, 63)) == (
        "variant 1 (column codes) register 2 lane 63")


def test_aggregate_clean_and_empty(movement_exe):
    rows = [(x, _hw(x & 7, 0, cu, s), 0, 0, 0xFFFFFFFF, 0, 1)
            for x in range(8) for cu in range(3) for s in range(4)]
    got, name = _both(movement_exe, rows)
    assert got["waves_run"] == 96 and got["cus_seen"] == 24 and got["simds_seen"] == 96
    assert got["xcds_seen"] == 8 and got["waves_bad"] == 0 and got["first_bad_index"] == -1
    assert got["xcd"] == -1 and got["first_bad"] == 0xFFFFFFFF and name == ""
    got, _ = _both(movement_exe, [(0, 0, 1, 1, 1, 1, 0)])
    assert got["waves_run"] == 0 and got["fail_mask"] == 0


# -- the stage's assembly ----------------------------------------------------------------------------


@pytest.fixture(scope="module")
def stage_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("movement-asm") / "movement.s"
    subprocess.run([hip_build.HIPCC, *hip_build.DEVICE_FLAGS, "-S", "--cuda-device-only",
                    hip_build.MOVEMENT_SRC, "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    start = text.index("movement_kernel")
    end = text.index(".end_amdhsa_kernel", start)
    return text[start:end]


def test_stage_kernel_holds_every_instruction_under_test(stage_asm):
    body = stage_asm
    dpp_controls = ["quad_perm:[1,3,0,2]", "row_shl:1 ", "row_shr:3 ", "row_ror:5 ", "row_mirror",
                    "row_half_mirror", "wave_shl:1", "wave_shr:1", "wave_rol:1", "wave_ror:1",
                    "row_bcast:15 row_mask:0xa", "row_bcast:31 row_mask:0xc"]
    for control in dpp_controls:
        assert re.search(r"_dpp .*" + re.escape(control), body), control
    assert re.search(r"_dpp .*row_shr:1 row_mask:0xf bank_mask:0x5", body)
    assert len(re.findall(r"_dpp .*bound_ctrl:1", body)) == 2
    counts = {m: len(re.findall(r"\b" + m + r"\b", body)) for m in (
        "ds_swizzle_b32", "ds_permute_b32", r"v_permlane16_swap_b32\w*", r"v_permlane32_swap_b32\w*",
        "ds_read_b64_tr_b16", "ds_read_b64_tr_b8", "ds_read_b64_tr_b4", "ds_read_b96_tr_b6",
        "global_load_lds_dword", "global_load_lds_dwordx4")}
    assert counts["ds_swizzle_b32"] == 5
    assert counts["ds_permute_b32"] == 1
    assert counts[r"v_permlane16_swap_b32\w*"] == 1 and counts[r"v_permlane32_swap_b32\w*"] == 1
    for tr in ("ds_read_b64_tr_b16", "ds_read_b64_tr_b8", "ds_read_b64_tr_b4", "ds_read_b96_tr_b6"):
        assert counts[tr] == 2, tr
    assert counts["global_load_lds_dword"] == 2 and counts["global_load_lds_dwordx4"] == 1
    assert re.search(r"global_load_lds_dword v\[\d+:\d+\], off offset:64", body)
    assert len(re.findall(r"\bds_bpermute_b32\b", body)) >= 2
    assert len(re.findall(r"\bv_readlane_b32\b", body)) >= 2
    assert len(re.findall(r"\bv_readfirstlane_b32\b", body)) >= 2
    assert re.search(r"s_nop 4\n\s*v_writelane_b32 v\d+, s\d+, m0", body)
    # the partial-EXEC v_readfirstlane sits inside a saved-EXEC region
    assert re.search(r"s_and_saveexec_b64[^\n]*\n(?:[^\n]*\n){1,12}?\s*v_readfirstlane_b32", body)
    # the DMA is waited for before the barrier that precedes the read-back
    assert re.search(r"global_load_lds_dwordx4[^\n]*\n(?:[^\n]*\n){0,8}?\s*s_waitcnt vmcnt\(0\)"
                     r"[^\n]*\n\s*s_barrier", body)


def test_stage_kernel_uses_no_scratch(stage_asm):
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", stage_asm)
    assert "scratch_" not in stage_asm.replace("uses_flat_scratch", "")


# -- plumbing ----------------------------------------------------------------------------------------


class Gpu:
    pci_bdf = "0000:05:00.0"


GOOD_QUICK = {"ok": True, "rc": 0, "mfma_f32_exact": True, "hbm_gbps": 4000.0, "msg": "ok"}
GOOD_STAGE = {
    "ok": True, "rc": 0, "cus_expected": 256, "cus_seen": 256, "xcds_seen": 8,
    "simds_seen": 1024, "rounds": 1, "waves_run": 1024, "waves_bad": 0, "cus_bad": 0,
    "failed_test": "", "gpu_ms": 0.134, "msg": "ok",
}
GOOD_COHERENCE = dict(GOOD_STAGE, pairs_checked=16128, tally_level=-1)
GOOD_MOVEMENT = dict(GOOD_STAGE, gpu_ms=0.26, first_bad=0xFFFFFFFF)
BAD_MOVEMENT = dict(GOOD_MOVEMENT, ok=False, rc=-36, failed_test="dpp", xcd=5, se=2, sh=0, cu=7,
                    simd=3, waves_bad=4, cus_bad=1, first_bad=M.movement_elem(3, 0, 17),
                    bits_bad=0x00010000, msg="data-movement mismatch in dpp")
GOOD_INTEGRITY = {
    "ok": True, "rc": 0, "n_bad": 0, "failed_stage": "", "msg": "ok",
    "vram_passes": 2, "vram_bytes_verified": 2 << 30,
    "h2d_dma_bytes_verified": 256 << 20, "d2h_dma_bytes_verified": 256 << 20,
    "h2d_dma_gbps": 51.5, "d2h_dma_gbps": 49.0,
}


def _patch_probe(monkeypatch, quick=GOOD_QUICK, compute=GOOD_STAGE, formats=GOOD_STAGE,
                 coherence=GOOD_COHERENCE, movement=GOOD_MOVEMENT, integrity=GOOD_INTEGRITY):
    from cro_amd.nodeops import coherence as C
    from cro_amd.nodeops import formats as F

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
    monkeypatch.setattr(C, "run_coherence", runner("coherence", coherence))
    monkeypatch.setattr(M, "run_movement", runner("movement", movement))
    monkeypatch.setattr(probe_mod, "run_integrity", runner("integrity", integrity))
    return order


def _stages(order):
    return [name for name, _, _ in order]


def test_movement_off_returns_todays_hooks(monkeypatch):
    assert probe_mod.make_probe_fn("quick", movement=False) is probe_mod.probe_fn_for_nodeops
    order = _patch_probe(monkeypatch)
    fn = probe_mod.make_probe_fn("deep", compute=True, formats=True, coherence=True,
                                 movement=False)
    assert fn(Gpu()) == dict(GOOD_QUICK, compute=GOOD_STAGE, formats=GOOD_STAGE,
                             coherence=GOOD_COHERENCE, integrity=GOOD_INTEGRITY)
    assert _stages(order) == ["quick", "compute", "formats", "coherence", "integrity"]
    assert not hasattr(fn, "movement")


def test_stage_order_and_result(monkeypatch):
    order = _patch_probe(monkeypatch)
    fn = probe_mod.make_probe_fn("deep", compute=True, formats=True, coherence=True,
                                 movement=True, seed=9, movement_min_cu_fraction=0.5)
    result = fn(Gpu())
    assert _stages(order) == ["quick", "compute", "formats", "coherence", "movement", "integrity"]
    assert all(device == 3 for _, device, _ in order)
    assert order[4][2] == {"seed": 9, "min_cu_fraction": 0.5}
    assert list(result)[-5:] == ["compute", "formats", "coherence", "movement", "integrity"]
    assert result["ok"] is True
    order.clear()
    quick = probe_mod.make_probe_fn("quick", movement=True)
    assert quick(Gpu()) == dict(GOOD_QUICK, movement=GOOD_MOVEMENT) and quick.movement is True
    assert _stages(order) == ["quick", "movement"]


def test_stops_at_the_first_failing_stage(monkeypatch):
    fn = probe_mod.make_probe_fn("deep", compute=True, formats=True, coherence=True,
                                 movement=True)
    order = _patch_probe(monkeypatch, coherence=dict(GOOD_COHERENCE, ok=False, msg="c"))
    result = fn(Gpu())
    assert _stages(order) == ["quick", "compute", "formats", "coherence"]
    assert "movement" not in result and result["msg"] == "c"
    order = _patch_probe(monkeypatch, movement=BAD_MOVEMENT)
    result = fn(Gpu())
    assert _stages(order) == ["quick", "compute", "formats", "coherence", "movement"]
    assert result["ok"] is False and result["msg"] == BAD_MOVEMENT["msg"]
    assert result["movement"] == BAD_MOVEMENT and "integrity" not in result
    order = _patch_probe(monkeypatch, integrity=dict(GOOD_INTEGRITY, ok=False, msg="i"))
    result = fn(Gpu())
    assert _stages(order)[-2:] == ["movement", "integrity"]
    assert result["msg"] == "i" and result["movement"] == GOOD_MOVEMENT


def test_run_movement_builds_its_options(monkeypatch):
    seen = {}

    class Lib:
        @staticmethod
        def cro_movement_run(device, opts, res):
            o = ctypes.cast(opts, ctypes.POINTER(M.CroMovementOpts)).contents
            seen.update({name: getattr(o, name) for name, _ in M.CroMovementOpts._fields_})
            seen["device"] = device
            return -37

    monkeypatch.setattr(M, "load_movement_library", lambda required=None: Lib)
    out = M.run_movement(2, grid_blocks=3, iters=5, max_rounds=2, seed=-1, min_cu_fraction=0.25,
                         selftest_mode=1, selftest_test="lds_tr6", selftest_bit=30,
                         selftest_elem=M.movement_elem(1, 2, 63), selftest_key=0x50700,
                         selftest_also="lds_dma")
    assert seen == {"device": 2, "grid_blocks": 3, "iters": 5, "max_rounds": 2,
                    "seed": 0xFFFFFFFF, "selftest_mode": 1, "selftest_test": 8,
                    "selftest_bit": 30, "selftest_elem": (1 << 12) | (2 << 6) | 63,
                    "selftest_key": 0x50700, "selftest_also": 10, "min_cu_fraction": 0.25}
    assert out["ok"] is False and out["rc"] == -37 and list(out)[:2] == ["ok", "rc"]
    assert [k for k in out if k.startswith("bad_")] == [f"bad_{n}" for n in M.MOVEMENT_TESTS]
    with pytest.raises(TypeError):
        M.run_movement(0, lds_bytes=1)


def test_loader_without_the_library(monkeypatch, tmp_path):
    monkeypatch.setattr(M, "_lib", None)
    monkeypatch.setattr(M, "_LIB_PATH", str(tmp_path / "libcromovement.so"))
    assert M.load_movement_library(required=False) is None
    with pytest.raises(RuntimeError, match="libcromovement.so missing"):
        M.load_movement_library(required=True)
    with pytest.raises(RuntimeError):
        M.run_movement(0)  # never a silent pass
    with pytest.raises(RuntimeError):
        M.movement_tile(0, "dpp", 0, np.zeros((2, 64), dtype=np.uint32))


class RecordingExec:
    def __init__(self, stdout):
        self.stdout, self.argvs = stdout, []

    def run(self, node, argv, timeout=0):
        self.argvs.append(list(argv))
        return 0, self.stdout, ""


def test_exec_probe_argv_with_and_without_movement():
    ex = RecordingExec('{"ok": true, "movement": {"ok": true}}')
    base = ["croagent", "probe", "--bdf", "0000:05:00.0"]
    probe_mod.probe_via_exec(ex, "n0", Gpu())
    probe_mod.probe_via_exec(ex, "n0", Gpu(), movement=False, movement_min_cu_fraction=0.9)
    assert probe_mod.probe_via_exec(ex, "n0", Gpu(), movement=True)["movement"]["ok"] is True
    probe_mod.probe_via_exec(ex, "n0", Gpu(), movement=True, movement_min_cu_fraction=0.9)
    probe_mod.probe_via_exec(ex, "n0", Gpu(), level="deep", vram_mib=64, compute=True,
                             formats=True, coherence=True, movement=True)
    probe_mod.make_exec_probe_fn(ex, "n0", argv_prefix_fn=lambda: ["chroot", "/d"],
                                 movement=True, movement_min_cu_fraction=1)(Gpu())
    probe_mod.make_exec_probe_fn(ex, "n0", coherence=True)(Gpu())
    assert ex.argvs == [
        base,
        base,
        base + ["--movement"],
        base + ["--movement", "--movement-min-cu-fraction", "0.9"],
        base + ["--deep", "--vram-mib", "64", "--compute", "--formats", "--coherence",
                "--movement"],
        ["chroot", "/d"] + base + ["--movement", "--movement-min-cu-fraction", "1.0"],
        base + ["--coherence"],
    ]
    assert probe_mod._movement_argv(False, 0.5) == []


def test_a_stage_that_is_off_passes_no_keyword_of_its_own(monkeypatch):
    seen = []
    monkeypatch.setattr(probe_mod, "probe_via_exec",
                        lambda execer, node, gpu, **kw: seen.append(sorted(kw)) or {})
    probe_mod.make_exec_probe_fn(None, "n0")(Gpu())
    probe_mod.make_exec_probe_fn(None, "n0", movement=True)(Gpu())
    today = ["argv_prefix", "compute", "compute_min_cu_fraction", "level", "link_floor_gbps",
             "link_mib", "vram_mib"]
    assert seen == [today, sorted(today + ["movement", "movement_min_cu_fraction"])]


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


def test_controller_names_check_variant_lane_register_and_place(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, ok=False, formats=GOOD_STAGE, movement=BAD_MOVEMENT))
    metrics = mock_world.resource_rec.metrics
    counter = metrics.probe_movement_failures_total.labels(test="dpp")
    formats_counter = metrics.probe_formats_failures_total.labels(test="unknown")
    before, formats_before = counter._value.get(), formats_counter._value.get()
    with pytest.raises(FabricError):
        mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Attaching"
    assert got.status.error.startswith(
        "gfx950 health probe failed: movement stage dpp variant 3 (row_ror:5) register 0 "
        "lane 17 xcd=5 se=2 cu=7 simd=3 bits_bad=0x00010000 cus_bad=1: "
    ), got.status.error
    assert counter._value.get() == before + 1
    assert formats_counter._value.get() == formats_before


def test_controller_counts_the_coverage_floor(mock_world):
    floor = dict(GOOD_MOVEMENT, ok=False, rc=-37, msg="coverage 3 of 256 CUs")
    _attach(mock_world, dict(GOOD_QUICK, ok=False, movement=floor))
    counter = mock_world.resource_rec.metrics.probe_movement_failures_total.labels(
        test="coverage")
    before = counter._value.get()
    with pytest.raises(FabricError):
        mock_world.resource_rec.reconcile("gpu-1")
    assert counter._value.get() == before + 1
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.error.startswith(
        "gfx950 health probe failed: movement stage coverage xcd=None"), got.status.error


def test_controller_online_event_carries_the_movement_clause(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, formats=GOOD_STAGE, movement=GOOD_MOVEMENT,
                             integrity=GOOD_INTEGRITY))
    mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Online"
    assert _online_message(mock_world) == (
        f"device {got.status.device_id} online with CDI spec"
        "; probe: mfma_exact=True hbm=4000 GB/s"
        "; formats: 256/256 CUs, 1024 SIMDs, 0.1 ms"
        "; movement: 256/256 CUs, 1024 SIMDs, 0.3 ms"
        "; integrity: vram 1.00 GiB link 0.25 GiB verified, h2d 51.5 d2h 49.0 GB/s"
    )


def test_controller_messages_unchanged_without_a_movement_object(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, formats=GOOD_STAGE))
    mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert _online_message(mock_world) == (
        f"device {got.status.device_id} online with CDI spec"
        "; probe: mfma_exact=True hbm=4000 GB/s"
        "; formats: 256/256 CUs, 1024 SIMDs, 0.1 ms"
    )


def test_metrics_reset_unregisters_the_movement_counter():
    from prometheus_client import REGISTRY

    from cro_amd.metrics import Metrics

    Metrics()
    assert "cro_probe_movement_failures" in REGISTRY._names_to_collectors
    Metrics._reset_for_tests()
    try:
        assert "cro_probe_movement_failures" not in REGISTRY._names_to_collectors
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
                 "CRO_PROBE_FORMATS", "CRO_PROBE_FORMATS_MIN_CU_FRACTION",
                 "CRO_PROBE_COHERENCE", "CRO_PROBE_COHERENCE_MIN_CU_FRACTION",
                 "CRO_PROBE_MOVEMENT", "CRO_PROBE_MOVEMENT_MIN_CU_FRACTION"):
        monkeypatch.delenv(name, raising=False)


def test_entrypoint_movement_default_off_passes_todays_keywords(monkeypatch):
    from cro_amd.cmd import main as main_mod

    _clear_env(monkeypatch)
    args = _parse([])
    assert args.probe_movement == "off" and args.probe_movement_min_cu_fraction == 0
    assert main_mod.select_probe_fn(args) is probe_mod.probe_fn_for_nodeops
    seen = {}
    monkeypatch.setattr(probe_mod, "make_probe_fn", lambda level, **kw: seen.update(kw))
    main_mod.select_probe_fn(_parse(["--probe-coherence", "on"]))
    assert sorted(seen) == ["coherence", "coherence_min_cu_fraction", "compute",
                            "compute_min_cu_fraction", "link_bytes", "link_floor_gbps",
                            "vram_bytes"]


def test_entrypoint_flag_and_env_select_movement(monkeypatch):
    from cro_amd.cmd.main import select_probe_fn

    _clear_env(monkeypatch)
    fn = select_probe_fn(_parse(["--probe-movement", "on",
                                 "--probe-movement-min-cu-fraction", "0.75"]))
    assert fn.level == "quick" and fn.movement is True and fn.compute is False
    order = _patch_probe(monkeypatch)
    assert fn(Gpu())["movement"] == GOOD_MOVEMENT and _stages(order) == ["quick", "movement"]
    assert order[1][2]["min_cu_fraction"] == 0.75
    with pytest.raises(SystemExit):
        _parse(["--probe-movement", "maybe"])
    monkeypatch.setenv("CRO_PROBE_MOVEMENT", "on")
    monkeypatch.setenv("CRO_PROBE_MOVEMENT_MIN_CU_FRACTION", "0.5")
    args = _parse([])
    assert args.probe_movement == "on" and args.probe_movement_min_cu_fraction == 0.5
    assert select_probe_fn(args).movement is True
    # the flag wins over the environment
    assert select_probe_fn(_parse(["--probe-movement", "off"])) is probe_mod.probe_fn_for_nodeops


def test_a_missing_library_warns_and_switches_the_stage_off(monkeypatch, caplog):
    from cro_amd.cmd.main import drop_unavailable_probe_stages, select_probe_fn

    _clear_env(monkeypatch)
    log = logging.getLogger("test-movement")
    args = _parse(["--probe-movement", "on"])
    monkeypatch.setattr(M, "load_movement_library", lambda required=None: object())
    with caplog.at_level(logging.INFO, logger="test-movement"):
        assert drop_unavailable_probe_stages(args, log) is False
    assert args.probe_movement == "on" and "data-movement stage: on" in caplog.text
    caplog.clear()
    monkeypatch.setattr(M, "load_movement_library", lambda required=None: None)
    with caplog.at_level(logging.INFO, logger="test-movement"):
        assert drop_unavailable_probe_stages(args, log) is True
    assert args.probe_movement == "off"
    assert "data-movement probe library unavailable; movement stage disabled" in caplog.text
    assert select_probe_fn(args) is probe_mod.probe_fn_for_nodeops

    def broken(required=None):
        raise OSError("cannot load")

    args = _parse(["--probe-movement", "on"])
    monkeypatch.setattr(M, "load_movement_library", broken)
    assert drop_unavailable_probe_stages(args, log) is True and args.probe_movement == "off"
    caplog.clear()
    assert drop_unavailable_probe_stages(_parse([]), log) is False and caplog.text == ""


# -- croagent ------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def agent():
    if not os.path.exists(AGENT) or not os.path.exists(hip_build.OUT):
        hip_build.build()
    if not os.path.exists(hip_build.MOVEMENT_OUT):
        hip_build.build_movement()
    return AGENT


def test_croagent_probe_movement_without_a_gpu_leaves_no_trace(agent):
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present: the GPU tests run the stage itself")
    run = subprocess.run([agent, "probe", "--movement", "--movement-min-cu-fraction", "0.5"],
                         capture_output=True, text=True, timeout=60)
    out = json.loads(run.stdout)
    assert run.returncode == 1 and out["ok"] is False and "movement" not in out, out
    plain = subprocess.run([agent, "probe"], capture_output=True, text=True, timeout=60)
    assert plain.stdout == run.stdout  # a stage that did not run leaves no trace


def test_croagent_probe_movement_without_the_library(agent, tmp_path, monkeypatch):
    """An agent built by the build's own recipe beside libcroprobe.so only:
    ``probe --movement`` names the library that is missing before anything
    runs, in the scrubs' shape."""
    (tmp_path / "agent").mkdir()
    (tmp_path / "hip").mkdir()
    lone = tmp_path / "agent" / "croagent"
    shutil.copy(hip_build.OUT, tmp_path / "hip" / "libcroprobe.so")
    monkeypatch.setattr(hip_build, "HIP_DIR", str(tmp_path / "hip"))
    monkeypatch.setattr(hip_build, "AGENT_OUT", str(lone))
    hip_build.build_agent(force=True)
    run = subprocess.run([str(lone), "probe", "--movement"], capture_output=True, text=True,
                         timeout=60)
    (line,) = run.stdout.strip().splitlines()
    out = json.loads(line)
    assert run.returncode == 1 and set(out) == {"ok", "rc", "msg"}, out
    assert out["ok"] is False and out["rc"] == -1
    assert out["msg"].startswith("libcromovement.so not available: ")
    shutil.copy(hip_build.MOVEMENT_OUT, tmp_path / "hip" / "libcromovement.so")
    again = subprocess.run([str(lone), "probe", "--movement"], capture_output=True, text=True,
                           timeout=60)
    assert "libcromovement.so not available" not in again.stdout


# -- build --------------------------------------------------------------------------------------------------


def test_build_movement_inputs_staleness_and_command(tmp_path, monkeypatch):
    inputs = [hip_build.MOVEMENT_SRC] + hip_build.MOVEMENT_HEADERS
    assert {os.path.basename(p) for p in inputs} == {
        "movement.hip", "cromovement.h", "crohost.h", "crocoverage.h"}
    assert all(os.path.exists(p) for p in inputs)
    assert os.path.basename(hip_build.MOVEMENT_OUT) == "libcromovement.so"
    # the other libraries' lists have not learned the new files
    others = (hip_build.ALL_SRCS + hip_build.ALL_HEADERS + hip_build.SCRUB_HEADERS
              + hip_build.LDS_SCRUB_HEADERS + hip_build.REG_SCRUB_HEADERS
              + hip_build.FORMATS_HEADERS + hip_build.COHERENCE_HEADERS)
    assert not {"movement.hip", "cromovement.h"} & {os.path.basename(p) for p in others}
    assert [os.path.basename(p) for p in hip_build.ALL_SRCS] == [
        "probe.hip", "integrity.hip", "coverage.hip"]
    assert [os.path.basename(p) for p in hip_build.COHERENCE_HEADERS] == [
        "crocoherence.h", "crohost.h", "crocoverage.h"]
    assert [os.path.basename(p) for p in hip_build.FORMATS_HEADERS] == [
        "croformats.h", "crohost.h", "cromfma.h", "crocoverage.h"]
    files = {}
    for name in ("movement.hip", "cromovement.h", "crohost.h", "crocoverage.h", "probe.hip",
                 "crocoherence.h", "croagent.cpp"):
        files[name] = tmp_path / name
        files[name].write_text("")
        os.utime(files[name], (100, 100))
    out = tmp_path / "libcromovement.so"
    monkeypatch.setattr(hip_build, "MOVEMENT_SRC", str(files["movement.hip"]))
    monkeypatch.setattr(hip_build, "MOVEMENT_HEADERS", [
        str(files[n]) for n in ("cromovement.h", "crohost.h", "crocoverage.h")])
    monkeypatch.setattr(hip_build, "MOVEMENT_OUT", str(out))
    commands = []

    def fake_run(argv, check=True):
        commands.append(argv)
        target = argv[argv.index("-o") + 1]
        open(target, "a").close()
        os.utime(target, (400, 400))

    monkeypatch.setattr(hip_build.subprocess, "run", fake_run)
    assert hip_build.build_movement() == str(out)  # missing: built
    assert commands == [[hip_build.HIPCC, *hip_build.DEVICE_FLAGS, "-fPIC", "-shared",
                         str(files["movement.hip"]), "-o", str(out)]]
    commands.clear()
    hip_build.build_movement()
    assert commands == []  # up to date
    for name in ("movement.hip", "cromovement.h", "crohost.h", "crocoverage.h"):
        os.utime(out, (200, 200))
        os.utime(files[name], (300, 300))
        hip_build.build_movement()
        assert len(commands) == 1, name
        commands.clear()
        os.utime(files[name], (100, 100))
    os.utime(out, (200, 200))
    for name in ("probe.hip", "crocoherence.h", "croagent.cpp"):
        os.utime(files[name], (300, 300))  # not its inputs
    hip_build.build_movement()
    assert commands == []
    hip_build.build_movement(force=True)
    assert len(commands) == 1


def test_the_module_and_the_entry_build_the_movement_library(monkeypatch, capsys):
    import runpy

    built = []
    for name in ("build", "build_scrub", "build_lds_scrub", "build_reg_scrub", "build_formats",
                 "build_coherence", "build_movement"):
        monkeypatch.setattr(hip_build, name,
                            lambda force=False, name=name: built.append((name, force)) or name)
    entry = runpy.run_path(os.path.join(REPO, "__graft_entry__.py"))
    entry["build"]()
    assert built == [("build", True), ("build_scrub", True), ("build_lds_scrub", True),
                     ("build_reg_scrub", True), ("build_formats", True),
                     ("build_coherence", True), ("build_movement", True)]
    assert "built build_movement" in capsys.readouterr().out.splitlines()
    with open(hip_build.__file__) as f:
        main_block = f.read().split('if __name__ == "__main__":')[1]
    # after the stages' other libraries; the last line is pinned by an earlier test
    assert ('print(build_coherence(force="--force" in sys.argv))\n'
            '    print(build_movement(force="--force" in sys.argv))\n') in main_block
