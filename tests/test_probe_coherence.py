"""CPU tests of the coherence probe stage: the contributions, closed forms,
expected tally lines, payload hash and aggregation of crocoherence.h against
their numpy mirrors (through a small host program built with the host C++
compiler, also under the address and undefined-behaviour sanitizers: no HIP,
no GPU), the exactness bounds of the float tallies, the C structs against
their ctypes mirrors, and the plumbing from the operator flags down to the
agent."""

import argparse
import ctypes
import json
import logging
import os
import shutil
import subprocess

import numpy as np
import pytest

from cro_amd.api.v1alpha1.types import ComposableResource, Event
from cro_amd.fabric.base import FabricError
from cro_amd.hip import build as hip_build
from cro_amd.nodeops import coherence as C
from cro_amd.nodeops import probe as probe_mod
from tests.conftest import make_node, make_resource

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(REPO, "cro_amd", "hip")
AGENT = os.path.join(REPO, "cro_amd", "agent", "croagent")
SEEDS = (0, 0xDEADBEEF)
GRIDS = (1, 2, 63, 64, 65, C.MAX_GRID)


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

COHERENCE_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "crocoherence.h"

static void hex(const char* tag, const void* data, size_t n) {
  printf("%s ", tag);
  for (size_t i = 0; i < n; ++i) printf("%02x", ((const unsigned char*)data)[i]);
  printf("\n");
}

// the placement the tests use: round-robin, starting at XCD 3
static uint32_t xcc_of(int b) { return (uint32_t)((b + 3) % 8); }

static void print_agg(const CroCoherenceAgg& a) {
  printf("{\"waves_run\":%llu,\"waves_bad\":%llu,", a.waves_run, a.waves_bad);
  for (int t = 0; t < CRO_COH_TESTS; ++t) printf("\"bad_%s\":%llu,", kCroCohTestNames[t], a.bad[t]);
  printf("\"pairs_checked\":%llu,\"pairs_expected\":%llu,\"vis_bad\":%llu,\"vis_stale\":%llu,"
         "\"tally_got\":%llu,\"tally_want\":%llu,\"first_bad_index\":%lld,\"cus_seen\":%d,"
         "\"xcds_seen\":%d,\"simds_seen\":%d,\"cus_bad\":%d,\"xcd\":%d,\"se\":%d,\"sh\":%d,"
         "\"cu\":%d,\"simd\":%d,\"fail_mask\":%u,\"first_fail_mask\":%u,\"n_bad\":%u,"
         "\"first_bad\":%u,\"bits_bad\":%u,\"tally_level\":%d,\"tally_slot\":%d,"
         "\"tally_unit\":%d,\"tally_epoch\":%d,\"bad_block\":%d,\"ticket_slot\":%d,"
         "\"ticket_epoch\":%d,\"ticket_seen\":%u,\"ticket_owner\":%u,\"name\":\"%s\"}\n",
         a.pairs_checked, a.pairs_expected, a.vis_bad, a.vis_stale, a.tally_got, a.tally_want,
         a.first_bad_index, a.cus_seen, a.xcds_seen, a.simds_seen, a.cus_bad, a.xcd, a.se, a.sh,
         a.cu, a.simd, a.fail_mask, a.first_fail_mask, a.n_bad, a.first_bad, a.bits_bad,
         a.tally_level, a.tally_slot, a.tally_unit, a.tally_epoch, a.bad_block, a.ticket_slot,
         a.ticket_epoch, a.ticket_seen, a.ticket_owner, cro_coh_test_name(a.fail_mask));
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "totals")) {
    // closed form against the fold over every lane, every block of the grid
    const int grid = atoi(argv[2]);
    const unsigned seed = (unsigned)strtoul(argv[3], nullptr, 0);
    int differ = 0;
    for (unsigned epoch = 1; epoch <= 2; ++epoch)
      for (int wide = 0; wide < 2; ++wide)
        for (int b = 0; b < grid; ++b) {
          uint64_t a[CRO_COH_UNIT_WORDS], c[CRO_COH_UNIT_WORDS];
          CroCohTotals brute, closed;
          cro_coh_totals_init(&closed);
          cro_coh_block_totals_brute((uint32_t)b, cro_coh_salt(seed, epoch), wide, &brute);
          cro_coh_block_totals((uint32_t)b, cro_coh_salt(seed, epoch), wide, &closed);
          cro_coh_encode(&brute, a);
          cro_coh_encode(&closed, c);
          differ += memcmp(a, c, sizeof(a)) != 0;
        }
    printf("differ %d\n", differ);
    return 0;
  }
  if (!strcmp(argv[1], "units")) {
    const int grid = atoi(argv[2]);
    const unsigned seed = (unsigned)strtoul(argv[3], nullptr, 0);
    const unsigned epoch = (unsigned)atoi(argv[4]);
    std::vector<uint32_t> xcc(grid);
    for (int b = 0; b < grid; ++b) xcc[b] = xcc_of(b);
    std::vector<uint64_t> units((size_t)cro_coh_units(grid) * CRO_COH_UNIT_WORDS);
    cro_coh_initial_units(grid, units.data());
    hex("initial", units.data(), units.size() * 8);
    cro_coh_expected_units(grid, seed, epoch, xcc.data(), units.data());
    hex("expected", units.data(), units.size() * 8);
    uint32_t pay[4 * CRO_COH_PAYLOAD];
    for (int i = 0; i < 4 * CRO_COH_PAYLOAD; ++i)
      pay[i] = cro_coh_payload(seed, epoch, (uint32_t)(grid - 1 + i / CRO_COH_PAYLOAD),
                               (uint32_t)(i % CRO_COH_PAYLOAD));
    hex("payload", pay, sizeof(pay));
    printf("salt %u drop %u %u %u\n", cro_coh_salt(seed, epoch),
           cro_coh_drop_tid(CRO_COH_PK_F16, 77), cro_coh_drop_tid(CRO_COH_PK_BF16, 300),
           cro_coh_drop_tid(CRO_COH_ADD_U32, 5));
    return 0;
  }
  if (!strcmp(argv[1], "bounds")) {
    // the largest sum of |x| one slot can receive: 64 workgroups of the
    // largest grid on one shared line, and a workgroup's own line
    long long worst[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};  // [wide][f16, bf16, f32, f64]
    for (int wide = 0; wide < 2; ++wide)
      for (int sub = 0; sub < (wide ? CRO_COH_SUBS : CRO_COH_MAX_GRID); ++sub) {
        long long sum[4] = {0, 0, 0, 0};
        for (int b = 0; b < CRO_COH_MAX_GRID; ++b) {
          if (wide ? (int)cro_coh_sub((uint32_t)b) != sub : b != sub) continue;
          for (uint32_t tid = 0; tid < 256; ++tid) {
            uint32_t lo, hi;
            if (cro_coh_pk(0, wide, (uint32_t)b, tid, &lo, &hi)) sum[0] += lo > hi ? lo : hi;
            if (cro_coh_pk(1, wide, (uint32_t)b, tid, &lo, &hi)) sum[1] += lo > hi ? lo : hi;
            sum[2] += llabs((long long)cro_coh_v_f32((uint32_t)b, tid));
            sum[3] += llabs((long long)cro_coh_v_f64((uint32_t)b * 256u + tid));
          }
        }
        for (int k = 0; k < 4; ++k)
          if (sum[k] > worst[wide][k]) worst[wide][k] = sum[k];
      }
    for (int wide = 0; wide < 2; ++wide)
      printf("wide %d %lld %lld %lld %lld\n", wide, worst[wide][0], worst[wide][1],
             worst[wide][2], worst[wide][3]);
    return 0;
  }
  if (!strcmp(argv[1], "judge")) {
    // stdin: grid launches, then the records (16 words each), then per launch
    // "units" got / want words, "tickets" seen / owner words, "words"
    int grid = 0, launches = 0;
    if (scanf("%d %d", &grid, &launches) != 2) return 2;
    std::vector<CroCoherenceRecord> recs((size_t)grid * 4 * launches);
    for (auto& r : recs) {
      uint32_t* w = (uint32_t*)&r;
      for (int i = 0; i < 16; ++i)
        if (scanf("%u", &w[i]) != 1) return 2;
    }
    CroCoherenceAgg agg, host;
    cro_coherence_aggregate(recs.data(), grid, launches, &agg);
    cro_coherence_agg_clear(&host);
    const size_t uw = (size_t)cro_coh_units(grid) * CRO_COH_UNIT_WORDS;
    std::vector<uint64_t> got(uw), want(uw), words((grid + 63) / 64);
    std::vector<uint32_t> seen((size_t)grid * 256), owner((size_t)grid * 256);
    for (int l = 0; l < launches; ++l) {
      unsigned want_of_0 = 1;
      for (auto& x : got)
        if (scanf("%llu", (unsigned long long*)&x) != 1) return 2;
      for (auto& x : want)
        if (scanf("%llu", (unsigned long long*)&x) != 1) return 2;
      if (scanf("%u", &want_of_0) != 1) return 2;
      for (auto& x : seen)
        if (scanf("%u", &x) != 1) return 2;
      for (auto& x : owner)
        if (scanf("%u", &x) != 1) return 2;
      for (auto& x : words)
        if (scanf("%llu", (unsigned long long*)&x) != 1) return 2;
      const CroCoherenceRecord* lr = recs.data() + (size_t)l * grid * 4;
      cro_coh_check_tallies(got.data(), want.data(), grid, l + 1, lr, &host);
      cro_coh_check_tickets(seen.data(), owner.data(), grid, l + 1, want_of_0, lr, &host);
      cro_coh_check_words(words.data(), grid, &host);
    }
    print_agg(agg);
    cro_coh_agg_merge(&agg, &host);
    print_agg(agg);
    return 0;
  }
  if (!strcmp(argv[1], "sizes")) {
    printf("%zu %zu %zu %zu\n", sizeof(CroCoherenceOpts), sizeof(CroCoherenceRecord),
           sizeof(CroCoherenceAgg), sizeof(CroCoherenceResult));
    CroCoherenceResult r;
    printf("%zu %zu %zu %zu %zu\n", (size_t)((char*)&r.agg - (char*)&r),
           (size_t)((char*)&r.first_bad_round - (char*)&r), (size_t)((char*)&r.gpu_ms - (char*)&r),
           (size_t)((char*)&r.failed_test - (char*)&r), (size_t)((char*)&r.msg - (char*)&r));
    printf("%zu %zu %zu\n", (size_t)((char*)&r.agg.first_bad_index - (char*)&r),
           (size_t)((char*)&r.agg.tally_level - (char*)&r),
           (size_t)((char*)&r.agg.ticket_owner - (char*)&r));
    CroCoherenceOpts o;
    printf("%zu %zu\n", (size_t)((char*)&o.selftest_key - (char*)&o),
           (size_t)((char*)&o.min_cu_fraction - (char*)&o));
    for (int t = 0; t < CRO_COH_TESTS; ++t) printf("%s ", cro_coh_test_name(1u << t));
    printf("\n");
    return 0;
  }
  return 2;
}
"""


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def coherence_exe(request, tmp_path_factory):
    """The host program, plain and under the address and undefined-behaviour
    sanitizers (a stand-alone program: it needs nothing preloaded)."""
    extra = () if request.param == "plain" else (
        "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    return _build(tmp_path_factory.mktemp(f"coherence_{request.param}"), "coherence_main",
                  COHERENCE_MAIN, extra)


def _run(exe, *args, stdin=None):
    proc = subprocess.run([exe, *args], input=stdin, capture_output=True, text=True)
    assert proc.returncode == 0, (proc.returncode, proc.stderr[-3000:])
    return proc.stdout


def _xcc(grid):
    return [(b + 3) % 8 for b in range(grid)]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("grid", GRIDS)
def test_closed_forms_equal_the_fold_over_every_lane_in_the_header(coherence_exe, grid, seed):
    assert _run(coherence_exe, "totals", str(grid), str(seed)).split() == ["differ", "0"]


@pytest.mark.parametrize("seed", SEEDS)
def test_closed_forms_equal_the_fold_over_every_lane_in_numpy(seed):
    salt = C.coherence_salt(seed, 1)
    blocks = sorted({0, 1, 62, 63, 64, 255, 256, 300, C.MAX_GRID - 1})
    for wide in (0, 1):
        for b in blocks:
            assert C.block_totals(b, salt, wide) == C.block_totals_brute(b, salt, wide), (b, wide)
    # a dropped lane changes the totals by that lane's own amount
    v = C.lane_values(5, salt, 0)
    full, short = C.block_totals(5, salt, 0), C.block_totals_brute(5, salt, 0, skip="add_u32")
    assert (full["add32"] - short["add32"]) & 0xFFFFFFFF == int(v["add_u32"][0])
    short = C.block_totals_brute(77, salt, 1, skip="pk_add_f16")
    v = C.lane_values(77, salt, 1)
    tid = C.drop_tid("pk_add_f16", 77)
    assert v["f16_on"][tid] and v["f16_lo"][tid] != v["f16_hi"][tid]
    assert C.block_totals(77, salt, 1)["f16_lo"] - short["f16_lo"] == int(v["f16_lo"][tid])
    v16, v256 = C.lane_values(300, salt, 0), C.lane_values(300, salt, 1)
    tid = C.drop_tid("pk_add_bf16", 300)
    assert v16["bf16_on"][tid] and v256["bf16_on"][tid] and v16["f16_on"][C.drop_tid(4, 300)]
    # contributions above 2^32, top bits set in the min / max operands
    assert int(v["add_u64"].min()) > 1 << 32
    assert ((v["mm32"] >> 31) & 1).sum() == 128


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("grid", GRIDS)
def test_expected_units_and_payload_match_the_header(coherence_exe, grid, seed):
    lines = dict(line.split(" ", 1)
                 for line in _run(coherence_exe, "units", str(grid), str(seed), "2").splitlines())
    shape = (C.coherence_units(grid), C.UNIT_WORDS)
    initial = np.frombuffer(bytes.fromhex(lines["initial"]), dtype=np.uint64).reshape(shape)
    expected = np.frombuffer(bytes.fromhex(lines["expected"]), dtype=np.uint64).reshape(shape)
    assert np.array_equal(initial, C.initial_units(grid))
    assert np.array_equal(expected, C.expected_units(grid, seed, 2, _xcc(grid)))
    payload = np.frombuffer(bytes.fromhex(lines["payload"]), dtype=np.uint32)
    want = [C.payload_value(seed, 2, grid - 1 + i // 64, i % 64) for i in range(256)]
    assert payload.tolist() == want
    assert len(set(want)) == 256  # a hash, not a pattern
    salt, _, f16, bf16, other = lines["salt"].split()
    assert int(salt) == C.coherence_salt(seed, 2)
    assert [int(f16), int(bf16), int(other)] == [C.drop_tid(4, 77), C.drop_tid(5, 300), 0]


def test_exactness_bounds_hold_at_the_largest_grid(coherence_exe):
    rows = [list(map(int, line.split()[2:])) for line in _run(coherence_exe, "bounds").splitlines()]
    for f16, bf16, f32, f64 in rows:
        assert f16 <= 2048 and bf16 <= 256 and f32 < 2 ** 24 and f64 < 2 ** 53
    # and in numpy, with every block of a sub-slot on one line
    salt = C.coherence_salt(0, 1)
    worst = {"f16": 0, "bf16": 0, "f32": 0, "f64": 0}
    for sub in range(C.SUBS):
        total = dict.fromkeys(worst, 0)
        for b in range(C.MAX_GRID):
            if C.sub_slot(b) != sub:
                continue
            v = C.lane_values(b, salt, 1)
            total["f16"] += int(np.maximum(v["f16_lo"], v["f16_hi"]).sum())
            total["bf16"] += int(np.maximum(v["bf16_lo"], v["bf16_hi"]).sum())
            total["f32"] += int(np.abs(v["add_f32"]).sum())
            total["f64"] += int(np.abs(v["add_f64"]).sum())
        worst = {k: max(worst[k], total[k]) for k in worst}
    assert [worst[k] for k in ("f16", "bf16", "f32", "f64")] == rows[1]
    own = C.lane_values(C.MAX_GRID - 1, salt, 0)
    assert int(np.maximum(own["f16_lo"], own["f16_hi"]).sum()) <= 2048
    assert int(np.maximum(own["bf16_lo"], own["bf16_hi"]).sum()) <= 256


def _bf16_add(acc, x):
    """acc + x rounded to bf16 (round to nearest even), all float32."""
    s = np.float32(acc) + np.float32(x)
    bits = int(np.array(s, dtype=np.float32).view(np.uint32))
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return np.array(bits, dtype=np.uint32).view(np.float32)[()]


def test_float_totals_do_not_depend_on_the_order_of_summation():
    salt = C.coherence_salt(1, 1)
    blocks = [b for b in range(C.MAX_GRID) if C.sub_slot(b) == 7]  # one whole shared line
    vals = {k: [] for k in ("f32", "f16_lo", "f16_hi", "bf16_lo", "bf16_hi")}
    for b in blocks:
        v = C.lane_values(b, salt, 1)
        vals["f32"] += v["add_f32"].tolist()
        for name in ("f16", "bf16"):
            on = v[f"{name}_on"]
            vals[f"{name}_lo"] += v[f"{name}_lo"][on].tolist()
            vals[f"{name}_hi"] += v[f"{name}_hi"][on].tolist()
    rng = np.random.default_rng(7)
    for key, xs in vals.items():
        exact = sum(xs)
        orders = [xs, xs[::-1], [xs[i] for i in rng.permutation(len(xs))]]
        for order in orders:
            if key == "f32":
                acc = np.float32(0)
                for x in order:
                    acc = np.float32(acc + np.float32(x))
            elif key.startswith("f16"):
                acc = np.float16(0)
                for x in order:
                    acc = np.float16(acc + np.float16(x))
            else:
                acc = np.float32(0)
                for x in order:
                    acc = _bf16_add(acc, x)
            assert float(acc) == exact, (key, float(acc), exact)
    t = C.totals_init()
    for b in blocks:
        C.totals_fold(t, C.block_totals(b, salt, 1))
    assert (t["f32"], t["f16_lo"], t["bf16_hi"]) == (
        sum(vals["f32"]), sum(vals["f16_lo"]), sum(vals["bf16_hi"]))
    words = C.encode_totals(t)
    assert np.array([int(words[4]) & 0xFFFF], dtype=np.uint16).view(np.float16)[0] == t["f16_lo"]
    assert np.array([(int(words[5]) >> 16) << 16], dtype=np.uint32).view(np.float32)[0] == \
        t["bf16_hi"]


# -- aggregation of hand-made records ----------------------------------------------------


def _records(grid, launches):
    dtype = np.dtype([(name, np.uint32) for name in C.RECORD_FIELDS])
    rec = np.zeros(grid * 4 * launches, dtype=dtype)
    for i in range(rec.size):
        block, wave = (i // 4) % grid, i % 4
        xcd, cu = (block + 3) % 8, (block // 8) % 16
        rec["xcc_id"][i] = xcd
        rec["hw_id"][i] = (wave << 4) | (cu << 8) | ((block // 128) << 13)
        rec["valid"][i] = 1
        rec["block"][i] = block
        rec["vis_first_block"][i] = 0xFFFFFFFF
        rec["vis_first_dword"][i] = 0xFFFFFFFF
        rec["epoch"][i] = i // (grid * 4) + 1
    # arrival in block order: block b of a group sees b % 64 earlier ones
    for launch in range(launches):
        for b in range(grid):
            seen = b % 64
            for wave in range(4):
                rec["vis_pairs"][(launch * grid + b) * 4 + wave] = len(
                    [p for p in range(seen) if p % 4 == wave])
    return rec


def _judge(exe, rec, grid, launches, got, want, seen, owner, words, want_of_0=1):
    lines = [f"{grid} {launches}"]
    lines += [" ".join(str(int(r[k])) for k in C.RECORD_FIELDS) for r in rec]
    for launch in range(launches):
        lines.append(" ".join(str(int(x)) for x in got[launch].ravel()))
        lines.append(" ".join(str(int(x)) for x in want[launch].ravel()))
        lines.append(str(want_of_0))
        lines.append(" ".join(str(int(x)) for x in seen[launch]))
        lines.append(" ".join(str(int(x)) for x in owner[launch]))
        lines.append(" ".join(str(int(x)) for x in words[launch]))
    first, merged = _run(exe, "judge", stdin="\n".join(lines) + "\n").splitlines()
    return json.loads(first), json.loads(merged)


def _mirror(rec, grid, launches, got, want, seen, owner, words, want_of_0=1):
    agg = C.aggregate_coherence_records(rec, grid, launches)
    first = dict(agg)
    host = C.host_findings()
    for launch in range(launches):
        lr = rec[launch * grid * 4:(launch + 1) * grid * 4]
        C.check_tallies(got[launch], want[launch], grid, launch + 1, lr, host)
        C.check_tickets(seen[launch], owner[launch], grid, launch + 1, want_of_0, lr, host)
        C.check_words(words[launch], grid, host)
    C.merge_findings(agg, host)
    return first, agg


def _clean(grid, launches, seed=0):
    rec = _records(grid, launches)
    want = [C.expected_units(grid, seed, e + 1, _xcc(grid)) for e in range(launches)]
    got = [w.copy() for w in want]
    seen = [np.ones(grid * 256, dtype=np.uint32) for _ in range(launches)]
    owner = [np.arange(grid * 256, dtype=np.uint32)[::-1].copy() for _ in range(launches)]
    words = [np.array([(1 << min(64, grid - g0)) - 1 for g0 in range(0, grid, 64)],
                      dtype=np.uint64) for _ in range(launches)]
    return rec, got, want, seen, owner, words


def _same(exe, *args, **kw):
    header = _judge(exe, *args, **kw)
    mirror = _mirror(*args, **kw)
    for h, m in zip(header, mirror):
        name = h.pop("name")
        assert name == C.coherence_test_name(m["fail_mask"])
        assert h == m
    return mirror[1]


def test_aggregate_clean_counts_pairs_and_coverage(coherence_exe):
    grid, launches = 65, 2
    rec, got, want, seen, owner, words = _clean(grid, launches)
    agg = _same(coherence_exe, rec, grid, launches, got, want, seen, owner, words)
    assert agg["fail_mask"] == 0 and agg["waves_run"] == 65 * 4 * 2
    assert agg["pairs_checked"] == agg["pairs_expected"] == 2 * (64 * 63 // 2 + 0)
    assert agg["cus_seen"] == 65 and agg["xcds_seen"] == 8 and agg["simds_seen"] == 260
    assert agg["first_bad_index"] == -1 and agg["bad_block"] == -1 and agg["tally_level"] == -1


def test_aggregate_a_missing_arrival_bit_and_a_short_pair_count(coherence_exe):
    grid, launches = 65, 1
    rec, got, want, seen, owner, words = _clean(grid, launches)
    words[0][0] ^= np.uint64(1 << 17)  # block 17's bit never arrived in the word
    rec["vis_pairs"][40 * 4 + 1] -= 1  # and block 40 was not told of it
    agg = _same(coherence_exe, rec, grid, launches, got, want, seen, owner, words)
    assert agg["fail_mask"] == 1 << 11 and agg["bad_visibility"] == 2
    assert agg["pairs_checked"] == agg["pairs_expected"] - 1
    assert agg["waves_bad"] == 0 and agg["first_bad_index"] == -1


def test_aggregate_a_duplicate_ticket_names_who_drew_it(coherence_exe):
    grid, launches = 2, 2
    rec, got, want, seen, owner, words = _clean(grid, launches)
    seen[1][300], seen[1][301] = 2, 0  # a duplicate and the hole it leaves
    owner[1][300] = 256 + 70           # block 1, wave 1
    agg = _same(coherence_exe, rec, grid, launches, got, want, seen, owner, words)
    assert agg["fail_mask"] == 1 << 8 and agg["bad_ticket"] == 2
    assert (agg["ticket_slot"], agg["ticket_epoch"], agg["ticket_seen"]) == (300, 2, 2)
    assert agg["ticket_owner"] == 326 and agg["bad_block"] == 1
    assert (agg["xcd"], agg["cu"], agg["simd"]) == (4, 0, 1)


def test_aggregate_tally_levels_and_the_first_bad_record(coherence_exe):
    grid, launches = 65, 2
    rec, got, want, seen, owner, words = _clean(grid, launches)
    # a short workgroup line, its XCD line and its device line, epoch 2
    b = 41
    for unit in (b, C.xcd_unit(grid, (b + 3) % 8, b), C.dev_unit(grid, b)):
        got[1][unit, 2] -= np.uint64(1)
    # and a wave that failed lds_rmw and visibility in epoch 1
    i = 9 * 4 + 2
    rec["fail_mask"][i] = (1 << 10) | (1 << 11)
    rec["n_bad"][i], rec["first_bad"][i], rec["bits_bad"][i] = 1, 0, 8
    rec["vis_bad"][i], rec["vis_stale"][i] = 3, 1
    rec["vis_first_block"][i], rec["vis_first_dword"][i] = 6, 5
    first, merged = _judge(coherence_exe, rec, grid, launches, got, want, seen, owner, words)
    agg = _same(coherence_exe, rec, grid, launches, got, want, seen, owner, words)
    assert first["name"] == "lds_rmw" and first["first_bad_index"] == i
    assert first["bad_block"] == 9  # the failing wave's own workgroup
    assert (first["xcd"], first["cu"], first["simd"]) == (4, 1, 2)
    assert first["vis_bad"] == 3 and first["vis_stale"] == 1  # stale against other bad values
    # the lowest failing check leads: the tally, named by its workgroup line
    assert merged["name"] == "add_f32" and agg["bad_add_f32"] == 3
    assert (agg["tally_level"], agg["tally_unit"], agg["tally_slot"], agg["tally_epoch"]) == (
        0, b, 2, 2)
    assert agg["tally_want"] - agg["tally_got"] == 1
    assert agg["bad_block"] == b and (agg["xcd"], agg["cu"], agg["simd"]) == (4, 5, -1)
    assert agg["first_bad_index"] == -1 and agg["bad_lds_rmw"] == 1
    # an XCD line alone names the XCD, a device line only the slot
    got[1][b, 2] += np.uint64(1)
    agg = _same(coherence_exe, _records(grid, launches), grid, launches, got, want, seen, owner,
                words)
    assert (agg["tally_level"], agg["tally_unit"], agg["xcd"], agg["cu"]) == (1, 4, 4, -1)
    got[1][C.xcd_unit(grid, 4, b), 2] += np.uint64(1)
    agg = _same(coherence_exe, _records(grid, launches), grid, launches, got, want, seen, owner,
                words)
    assert (agg["tally_level"], agg["tally_unit"], agg["xcd"]) == (2, C.sub_slot(b), -1)


def test_a_visibility_failure_names_the_producer_block(coherence_exe):
    grid, launches = 8, 1
    rec, got, want, seen, owner, words = _clean(grid, launches)
    for consumer in (5, 6):
        i = consumer * 4 + 3
        rec["fail_mask"][i] = 1 << 11
        rec["n_bad"][i] = rec["vis_bad"][i] = 1
        rec["first_bad"][i] = 3 * 64 + 5
        rec["vis_first_block"][i], rec["vis_first_dword"][i] = 3, 5
        rec["bits_bad"][i] = rec["vis_bits"][i] = 8
    agg = _same(coherence_exe, rec, grid, launches, got, want, seen, owner, words)
    assert C.coherence_test_name(agg["fail_mask"]) == "visibility"
    assert agg["bad_block"] == 3 and agg["bad_visibility"] == 2 and agg["cus_bad"] == 2
    assert agg["vis_bad"] == 2 and agg["vis_stale"] == 0


# -- struct layouts ------------------------------------------------------------------------


def test_struct_layouts_match_ctypes(coherence_exe):
    sizes, offsets, agg_offsets, opt_offsets, names = _run(coherence_exe, "sizes").splitlines()
    R = C.CroCoherenceResult
    assert list(map(int, sizes.split()))[:2] == [
        ctypes.sizeof(C.CroCoherenceOpts), ctypes.sizeof(C.CroCoherenceRecord)]
    assert int(sizes.split()[3]) == ctypes.sizeof(R)
    agg_size = sum(ctypes.sizeof(t) for _, t in C.COHERENCE_AGG_FIELDS)
    assert int(sizes.split()[2]) == agg_size and agg_size % 8 == 0
    assert list(map(int, offsets.split())) == [
        R.waves_run.offset, R.first_bad_round.offset, R.gpu_ms.offset, R.failed_test.offset,
        R.msg.offset]
    assert list(map(int, agg_offsets.split())) == [
        R.first_bad_index.offset, R.tally_level.offset, R.ticket_owner.offset]
    assert list(map(int, opt_offsets.split())) == [
        C.CroCoherenceOpts.selftest_key.offset, C.CroCoherenceOpts.min_cu_fraction.offset]
    assert tuple(names.split()) == C.COHERENCE_TESTS
    assert [C.coherence_test_name(1 << t) for t in range(12)] == list(C.COHERENCE_TESTS)
    assert C.coherence_test_name(0) == "" and C.coherence_test_name(0b1100) == "add_f32"
    assert ctypes.sizeof(C.CroCoherenceRecord) == 64


# -- plumbing ----------------------------------------------------------------------------------------


class Gpu:
    pci_bdf = "0000:05:00.0"


GOOD_QUICK = {"ok": True, "rc": 0, "mfma_f32_exact": True, "hbm_gbps": 4000.0, "msg": "ok"}
GOOD_STAGE = {
    "ok": True, "rc": 0, "cus_expected": 256, "cus_seen": 256, "xcds_seen": 8,
    "simds_seen": 1024, "rounds": 1, "waves_run": 1024, "waves_bad": 0, "cus_bad": 0,
    "failed_test": "", "gpu_ms": 0.134, "msg": "ok",
}
GOOD_COHERENCE = dict(GOOD_STAGE, waves_run=2048, pairs_checked=16128, pairs_expected=16128,
                      gpu_ms=0.45, tally_level=-1)
BAD_TALLY = dict(GOOD_COHERENCE, ok=False, rc=-34, failed_test="pk_add_bf16", xcd=5, se=2, sh=0,
                 cu=7, simd=-1, tally_level=0, tally_unit=41, tally_slot=5, tally_got=0x40804000,
                 tally_want=0x40804040, bad_block=41, msg="coherence mismatch in pk_add_bf16")
BAD_WAVE = dict(GOOD_COHERENCE, ok=False, rc=-34, failed_test="visibility", xcd=1, se=3, sh=0,
                cu=2, simd=1, waves_bad=2, cus_bad=2, bad_block=17,
                msg="coherence mismatch in visibility")
GOOD_INTEGRITY = {
    "ok": True, "rc": 0, "n_bad": 0, "failed_stage": "", "msg": "ok",
    "vram_passes": 2, "vram_bytes_verified": 2 << 30,
    "h2d_dma_bytes_verified": 256 << 20, "d2h_dma_bytes_verified": 256 << 20,
    "h2d_dma_gbps": 51.5, "d2h_dma_gbps": 49.0,
}


def _patch_probe(monkeypatch, quick=GOOD_QUICK, compute=GOOD_STAGE, formats=GOOD_STAGE,
                 coherence=GOOD_COHERENCE, integrity=GOOD_INTEGRITY):
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
    monkeypatch.setattr(probe_mod, "run_integrity", runner("integrity", integrity))
    return order


def _stages(order):
    return [name for name, _, _ in order]


def test_coherence_off_returns_todays_hooks(monkeypatch):
    assert probe_mod.make_probe_fn("quick", coherence=False) is probe_mod.probe_fn_for_nodeops
    order = _patch_probe(monkeypatch)
    fn = probe_mod.make_probe_fn("deep", compute=True, formats=True, coherence=False)
    assert fn(Gpu()) == dict(GOOD_QUICK, compute=GOOD_STAGE, formats=GOOD_STAGE,
                             integrity=GOOD_INTEGRITY)
    assert _stages(order) == ["quick", "compute", "formats", "integrity"]
    assert not hasattr(fn, "coherence")


def test_stage_order_and_result(monkeypatch):
    order = _patch_probe(monkeypatch)
    fn = probe_mod.make_probe_fn("deep", compute=True, formats=True, coherence=True, seed=9,
                                 coherence_min_cu_fraction=0.5)
    result = fn(Gpu())
    assert _stages(order) == ["quick", "compute", "formats", "coherence", "integrity"]
    assert all(device == 3 for _, device, _ in order)
    assert order[3][2] == {"seed": 9, "min_cu_fraction": 0.5}
    assert list(result)[-4:] == ["compute", "formats", "coherence", "integrity"]
    assert result["ok"] is True
    order.clear()
    quick = probe_mod.make_probe_fn("quick", coherence=True)
    assert quick(Gpu()) == dict(GOOD_QUICK, coherence=GOOD_COHERENCE) and quick.coherence is True
    assert _stages(order) == ["quick", "coherence"]


def test_stops_at_the_first_failing_stage(monkeypatch):
    fn = probe_mod.make_probe_fn("deep", compute=True, formats=True, coherence=True)
    order = _patch_probe(monkeypatch, formats=dict(GOOD_STAGE, ok=False, msg="f"))
    result = fn(Gpu())
    assert _stages(order) == ["quick", "compute", "formats"] and "coherence" not in result
    order = _patch_probe(monkeypatch, coherence=BAD_WAVE)
    result = fn(Gpu())
    assert _stages(order) == ["quick", "compute", "formats", "coherence"]
    assert result["ok"] is False and result["msg"] == BAD_WAVE["msg"]
    assert result["coherence"] == BAD_WAVE and "integrity" not in result
    order = _patch_probe(monkeypatch, integrity=dict(GOOD_INTEGRITY, ok=False, msg="i"))
    result = fn(Gpu())
    assert _stages(order)[-2:] == ["coherence", "integrity"]
    assert result["msg"] == "i" and result["coherence"] == GOOD_COHERENCE


def test_run_coherence_builds_its_options(monkeypatch):
    seen = {}

    class Lib:
        @staticmethod
        def cro_coherence_run(device, opts, res):
            o = ctypes.cast(opts, ctypes.POINTER(C.CroCoherenceOpts)).contents
            seen.update({name: getattr(o, name) for name, _ in C.CroCoherenceOpts._fields_})
            seen["device"] = device
            return -35

    monkeypatch.setattr(C, "load_coherence_library", lambda required=None: Lib)
    out = C.run_coherence(2, grid_blocks=3, iters=5, max_rounds=2, seed=-1, min_cu_fraction=0.25,
                          selftest_mode=2, selftest_test="lds_rmw", selftest_bit=30,
                          selftest_key=0x50700)
    assert seen == {"device": 2, "grid_blocks": 3, "iters": 5, "max_rounds": 2,
                    "seed": 0xFFFFFFFF, "selftest_mode": 2, "selftest_test": 10,
                    "selftest_bit": 30, "selftest_key": 0x50700, "min_cu_fraction": 0.25}
    assert out["ok"] is False and out["rc"] == -35 and list(out)[:2] == ["ok", "rc"]
    assert [k for k in out if k.startswith("bad_") and k != "bad_block"] == [
        f"bad_{n}" for n in C.COHERENCE_TESTS]
    with pytest.raises(TypeError):
        C.run_coherence(0, selftest_elem=1)


def test_loader_without_the_library(monkeypatch, tmp_path):
    monkeypatch.setattr(C, "_lib", None)
    monkeypatch.setattr(C, "_LIB_PATH", str(tmp_path / "libcrocoherence.so"))
    assert C.load_coherence_library(required=False) is None
    with pytest.raises(RuntimeError, match="libcrocoherence.so missing"):
        C.load_coherence_library(required=True)
    with pytest.raises(RuntimeError):
        C.run_coherence(0)  # never a silent pass


class RecordingExec:
    def __init__(self, stdout):
        self.stdout, self.argvs = stdout, []

    def run(self, node, argv, timeout=0):
        self.argvs.append(list(argv))
        return 0, self.stdout, ""


def test_exec_probe_argv_with_and_without_coherence():
    ex = RecordingExec('{"ok": true, "coherence": {"ok": true}}')
    base = ["croagent", "probe", "--bdf", "0000:05:00.0"]
    probe_mod.probe_via_exec(ex, "n0", Gpu())
    probe_mod.probe_via_exec(ex, "n0", Gpu(), coherence=False, coherence_min_cu_fraction=0.9)
    assert probe_mod.probe_via_exec(ex, "n0", Gpu(), coherence=True)["coherence"]["ok"] is True
    probe_mod.probe_via_exec(ex, "n0", Gpu(), coherence=True, coherence_min_cu_fraction=0.9)
    probe_mod.probe_via_exec(ex, "n0", Gpu(), level="deep", vram_mib=64, compute=True,
                             formats=True, coherence=True)
    probe_mod.make_exec_probe_fn(ex, "n0", argv_prefix_fn=lambda: ["chroot", "/d"],
                                 coherence=True, coherence_min_cu_fraction=1)(Gpu())
    probe_mod.make_exec_probe_fn(ex, "n0", formats=True)(Gpu())
    assert ex.argvs == [
        base,
        base,
        base + ["--coherence"],
        base + ["--coherence", "--coherence-min-cu-fraction", "0.9"],
        base + ["--deep", "--vram-mib", "64", "--compute", "--formats", "--coherence"],
        ["chroot", "/d"] + base + ["--coherence", "--coherence-min-cu-fraction", "1.0"],
        base + ["--formats"],
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


def test_controller_refuses_online_on_a_tally_failure(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, ok=False, formats=GOOD_STAGE, coherence=BAD_TALLY))
    metrics = mock_world.resource_rec.metrics
    counter = metrics.probe_coherence_failures_total.labels(test="pk_add_bf16")
    formats_counter = metrics.probe_formats_failures_total.labels(test="unknown")
    before, formats_before = counter._value.get(), formats_counter._value.get()
    with pytest.raises(FabricError):
        mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Attaching"
    assert got.status.error.startswith(
        "gfx950 health probe failed: coherence stage pk_add_bf16 xcd=5 se=2 cu=7 simd=-1 "
        "level=workgroup line=41 slot=5 got=0x40804000 want=0x40804040 block=41 cus_bad=0"
    ), got.status.error
    assert counter._value.get() == before + 1
    assert formats_counter._value.get() == formats_before


def test_controller_names_the_wave_of_a_visibility_failure(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, ok=False, coherence=BAD_WAVE))
    counter = mock_world.resource_rec.metrics.probe_coherence_failures_total.labels(
        test="visibility")
    before = counter._value.get()
    with pytest.raises(FabricError):
        mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.error.startswith(
        "gfx950 health probe failed: coherence stage visibility xcd=1 se=3 cu=2 simd=1 "
        "block=17 cus_bad=2"), got.status.error
    assert counter._value.get() == before + 1


def test_controller_counts_the_coverage_floor(mock_world):
    floor = dict(GOOD_COHERENCE, ok=False, rc=-35, msg="coverage 3 of 256 CUs")
    _attach(mock_world, dict(GOOD_QUICK, ok=False, coherence=floor))
    counter = mock_world.resource_rec.metrics.probe_coherence_failures_total.labels(
        test="coverage")
    before = counter._value.get()
    with pytest.raises(FabricError):
        mock_world.resource_rec.reconcile("gpu-1")
    assert counter._value.get() == before + 1


def test_controller_online_event_carries_the_coherence_clause(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, formats=GOOD_STAGE, coherence=GOOD_COHERENCE,
                             integrity=GOOD_INTEGRITY))
    mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Online"
    assert _online_message(mock_world) == (
        f"device {got.status.device_id} online with CDI spec"
        "; probe: mfma_exact=True hbm=4000 GB/s"
        "; formats: 256/256 CUs, 1024 SIMDs, 0.1 ms"
        "; coherence: 256/256 CUs, 16128 pairs, 0.5 ms"
        "; integrity: vram 1.00 GiB link 0.25 GiB verified, h2d 51.5 d2h 49.0 GB/s"
    )


def test_controller_messages_unchanged_without_a_coherence_object(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, formats=GOOD_STAGE))
    mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert _online_message(mock_world) == (
        f"device {got.status.device_id} online with CDI spec"
        "; probe: mfma_exact=True hbm=4000 GB/s"
        "; formats: 256/256 CUs, 1024 SIMDs, 0.1 ms"
    )


def test_metrics_reset_unregisters_the_coherence_counter():
    from prometheus_client import REGISTRY

    from cro_amd.metrics import Metrics

    Metrics()
    assert "cro_probe_coherence_failures" in REGISTRY._names_to_collectors
    Metrics._reset_for_tests()
    try:
        assert "cro_probe_coherence_failures" not in REGISTRY._names_to_collectors
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
                 "CRO_PROBE_COHERENCE", "CRO_PROBE_COHERENCE_MIN_CU_FRACTION"):
        monkeypatch.delenv(name, raising=False)


def test_entrypoint_coherence_default_off_passes_todays_keywords(monkeypatch):
    from cro_amd.cmd import main as main_mod

    _clear_env(monkeypatch)
    args = _parse([])
    assert args.probe_coherence == "off" and args.probe_coherence_min_cu_fraction == 0
    assert main_mod.select_probe_fn(args) is probe_mod.probe_fn_for_nodeops
    seen = {}
    monkeypatch.setattr(probe_mod, "make_probe_fn", lambda level, **kw: seen.update(kw))
    main_mod.select_probe_fn(_parse(["--probe-formats", "on"]))
    assert sorted(seen) == ["compute", "compute_min_cu_fraction", "formats",
                            "formats_min_cu_fraction", "link_bytes", "link_floor_gbps",
                            "vram_bytes"]


def test_entrypoint_flag_and_env_select_coherence(monkeypatch):
    from cro_amd.cmd.main import select_probe_fn

    _clear_env(monkeypatch)
    fn = select_probe_fn(_parse(["--probe-coherence", "on",
                                 "--probe-coherence-min-cu-fraction", "0.75"]))
    assert fn.level == "quick" and fn.coherence is True and fn.compute is False
    order = _patch_probe(monkeypatch)
    assert fn(Gpu())["coherence"] == GOOD_COHERENCE and _stages(order) == ["quick", "coherence"]
    assert order[1][2]["min_cu_fraction"] == 0.75
    with pytest.raises(SystemExit):
        _parse(["--probe-coherence", "maybe"])
    monkeypatch.setenv("CRO_PROBE_COHERENCE", "on")
    monkeypatch.setenv("CRO_PROBE_COHERENCE_MIN_CU_FRACTION", "0.5")
    args = _parse([])
    assert args.probe_coherence == "on" and args.probe_coherence_min_cu_fraction == 0.5
    assert select_probe_fn(args).coherence is True
    # the flag wins over the environment
    assert select_probe_fn(_parse(["--probe-coherence", "off"])) is probe_mod.probe_fn_for_nodeops


def test_a_missing_library_warns_and_switches_the_stage_off(monkeypatch, caplog):
    from cro_amd.cmd.main import drop_unavailable_probe_stages, select_probe_fn

    _clear_env(monkeypatch)
    log = logging.getLogger("test-coherence")
    args = _parse(["--probe-coherence", "on"])
    monkeypatch.setattr(C, "load_coherence_library", lambda required=None: object())
    with caplog.at_level(logging.INFO, logger="test-coherence"):
        assert drop_unavailable_probe_stages(args, log) is False
    assert args.probe_coherence == "on" and "coherence stage: on" in caplog.text
    caplog.clear()
    monkeypatch.setattr(C, "load_coherence_library", lambda required=None: None)
    with caplog.at_level(logging.INFO, logger="test-coherence"):
        assert drop_unavailable_probe_stages(args, log) is True
    assert args.probe_coherence == "off"
    assert "coherence probe library unavailable; coherence stage disabled" in caplog.text
    assert select_probe_fn(args) is probe_mod.probe_fn_for_nodeops

    def broken(required=None):
        raise OSError("cannot load")

    args = _parse(["--probe-coherence", "on"])
    monkeypatch.setattr(C, "load_coherence_library", broken)
    assert drop_unavailable_probe_stages(args, log) is True and args.probe_coherence == "off"
    caplog.clear()
    assert drop_unavailable_probe_stages(_parse([]), log) is False and caplog.text == ""


# -- croagent ------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def agent():
    if not os.path.exists(AGENT) or not os.path.exists(hip_build.OUT):
        hip_build.build()
    if not os.path.exists(hip_build.COHERENCE_OUT):
        hip_build.build_coherence()
    return AGENT


def test_croagent_probe_coherence_without_a_gpu_reports_the_quick_failure(agent):
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present: the GPU tests run the stage itself")
    run = subprocess.run([agent, "probe", "--coherence", "--coherence-min-cu-fraction", "0.5"],
                         capture_output=True, text=True, timeout=60)
    out = json.loads(run.stdout)
    assert run.returncode == 1 and out["ok"] is False and "coherence" not in out, out
    plain = subprocess.run([agent, "probe"], capture_output=True, text=True, timeout=60)
    assert plain.stdout == run.stdout  # a stage that did not run leaves no trace


def test_croagent_probe_coherence_without_the_library(agent, tmp_path, monkeypatch):
    """An agent built by the build's own recipe beside libcroprobe.so only:
    ``probe --coherence`` names the library that is missing before anything
    runs, in the scrubs' shape."""
    (tmp_path / "agent").mkdir()
    (tmp_path / "hip").mkdir()
    lone = tmp_path / "agent" / "croagent"
    shutil.copy(hip_build.OUT, tmp_path / "hip" / "libcroprobe.so")
    monkeypatch.setattr(hip_build, "HIP_DIR", str(tmp_path / "hip"))
    monkeypatch.setattr(hip_build, "AGENT_OUT", str(lone))
    hip_build.build_agent(force=True)
    run = subprocess.run([str(lone), "probe", "--coherence"], capture_output=True, text=True,
                         timeout=60)
    (line,) = run.stdout.strip().splitlines()
    out = json.loads(line)
    assert run.returncode == 1 and set(out) == {"ok", "rc", "msg"}, out
    assert out["ok"] is False and out["rc"] == -1
    assert out["msg"].startswith("libcrocoherence.so not available: ")
    shutil.copy(hip_build.COHERENCE_OUT, tmp_path / "hip" / "libcrocoherence.so")
    again = subprocess.run([str(lone), "probe", "--coherence"], capture_output=True, text=True,
                           timeout=60)
    assert "libcrocoherence.so not available" not in again.stdout


# -- build --------------------------------------------------------------------------------------------------


def test_build_coherence_inputs_staleness_and_command(tmp_path, monkeypatch):
    inputs = [hip_build.COHERENCE_SRC] + hip_build.COHERENCE_HEADERS
    assert {os.path.basename(p) for p in inputs} == {
        "coherence.hip", "crocoherence.h", "crohost.h", "crocoverage.h"}
    assert all(os.path.exists(p) for p in inputs)
    assert os.path.basename(hip_build.COHERENCE_OUT) == "libcrocoherence.so"
    # the other libraries' lists have not learned the new files
    others = (hip_build.ALL_SRCS + hip_build.ALL_HEADERS + hip_build.SCRUB_HEADERS
              + hip_build.LDS_SCRUB_HEADERS + hip_build.REG_SCRUB_HEADERS
              + hip_build.FORMATS_HEADERS)
    assert not {"coherence.hip", "crocoherence.h"} & {os.path.basename(p) for p in others}
    files = {}
    for name in ("coherence.hip", "crocoherence.h", "crohost.h", "crocoverage.h", "probe.hip",
                 "croformats.h", "croagent.cpp"):
        files[name] = tmp_path / name
        files[name].write_text("")
        os.utime(files[name], (100, 100))
    out = tmp_path / "libcrocoherence.so"
    monkeypatch.setattr(hip_build, "COHERENCE_SRC", str(files["coherence.hip"]))
    monkeypatch.setattr(hip_build, "COHERENCE_HEADERS", [
        str(files[n]) for n in ("crocoherence.h", "crohost.h", "crocoverage.h")])
    monkeypatch.setattr(hip_build, "COHERENCE_OUT", str(out))
    commands = []

    def fake_run(argv, check=True):
        commands.append(argv)
        target = argv[argv.index("-o") + 1]
        open(target, "a").close()
        os.utime(target, (400, 400))

    monkeypatch.setattr(hip_build.subprocess, "run", fake_run)
    assert hip_build.build_coherence() == str(out)  # missing: built
    assert commands == [[hip_build.HIPCC, *hip_build.DEVICE_FLAGS, "-fPIC", "-shared",
                         str(files["coherence.hip"]), "-o", str(out)]]
    commands.clear()
    hip_build.build_coherence()
    assert commands == []  # up to date
    for name in ("coherence.hip", "crocoherence.h", "crohost.h", "crocoverage.h"):
        os.utime(out, (200, 200))
        os.utime(files[name], (300, 300))
        hip_build.build_coherence()
        assert len(commands) == 1, name
        commands.clear()
        os.utime(files[name], (100, 100))
    os.utime(out, (200, 200))
    for name in ("probe.hip", "croformats.h", "croagent.cpp"):
        os.utime(files[name], (300, 300))  # not its inputs
    hip_build.build_coherence()
    assert commands == []
    hip_build.build_coherence(force=True)
    assert len(commands) == 1


def test_the_module_and_the_entry_build_the_coherence_library(monkeypatch, capsys):
    import runpy

    built = []
    for name in ("build", "build_scrub", "build_lds_scrub", "build_reg_scrub", "build_formats",
                 "build_coherence"):
        monkeypatch.setattr(hip_build, name,
                            lambda force=False, name=name: built.append((name, force)) or name)
    entry = runpy.run_path(os.path.join(REPO, "__graft_entry__.py"))
    entry["build"]()
    assert built == [("build", True), ("build_scrub", True), ("build_lds_scrub", True),
                     ("build_reg_scrub", True), ("build_formats", True),
                     ("build_coherence", True)]
    assert "built build_coherence" in capsys.readouterr().out.splitlines()
    with open(hip_build.__file__) as f:
        main_block = f.read().split('if __name__ == "__main__":')[1]
    assert 'print(build_coherence(force="--force" in sys.argv))' in main_block
