"""CPU tests of the deep (data-integrity) probe: the pattern and the two C
structs against their Python mirrors (through small host programs built with
the host C++ compiler — no HIP, no GPU), the probe-level plumbing, the
controller's handling of an integrity result, and the operator flags."""

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
        [_host_cxx(), "-std=c++17", "-O1", f"-I{HIP_DIR}", str(src), "-o", str(exe)],
        check=True, capture_output=True, text=True,
    )
    return str(exe)


# -- pattern ------------------------------------------------------------------

PATTERN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "cropattern.h"
int main(int argc, char** argv) {
  if (argc != 5) return 2;
  unsigned long long base = strtoull(argv[1], nullptr, 10), n = strtoull(argv[2], nullptr, 10);
  unsigned seed = (unsigned)strtoul(argv[3], nullptr, 10), invert = (unsigned)atoi(argv[4]);
  for (unsigned long long i = 0; i < n; ++i) printf("%u\n", cro_pattern_word(base + i, seed, invert));
  return 0;
}
"""


@pytest.fixture(scope="module")
def pattern_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pattern"), "pattern_main", PATTERN_MAIN)


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("base", [0, (1 << 32) - 5, (1 << 36) + 1])
def test_pattern_header_matches_numpy(pattern_exe, base, invert):
    seed, n = 0x1234ABCD, 37
    out = subprocess.run(
        [pattern_exe, str(base), str(n), str(seed), str(invert)],
        check=True, capture_output=True, text=True,
    ).stdout.split()
    host = np.array([int(v) for v in out], dtype=np.uint32)
    ref = probe_mod.pattern_words(base, n, seed, invert)
    assert ref.dtype == np.uint32 and ref.shape == (n,)
    assert np.array_equal(host, ref)


def test_pattern_inversion_is_complement():
    a = probe_mod.pattern_words(7, 100, 3, 0)
    b = probe_mod.pattern_words(7, 100, 3, 1)
    assert np.array_equal(a ^ b, np.full(100, 0xFFFFFFFF, dtype=np.uint32))


def test_pattern_first_2_20_words_distinct():
    """The final mix is a bijection, so no two addresses of a 2^32-word
    window share a value — what makes address aliasing visible."""
    words = probe_mod.pattern_words(0, 1 << 20, 0x1234ABCD, 0)
    assert np.unique(words).size == 1 << 20


# -- host-only header (crointegrity.h) --------------------------------------------

MIB = 1 << 20
SEED = 0x1234ABCD
SEED_BACK = SEED ^ 0xA5A5A5A5

INTEGRITY_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "crointegrity.h"
using namespace crointegrity;
static unsigned long long num(const char* s) { return strtoull(s, nullptr, 10); }
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const char* cmd = argv[1];
  if (!strcmp(cmd, "fill") && argc == 5) {  // n seed invert
    std::vector<uint32_t> buf(num(argv[2]));
    host_fill(buf.data(), buf.size(), (uint32_t)num(argv[3]), (uint32_t)num(argv[4]));
    for (uint32_t w : buf) printf("%u\n", w);
    return 0;
  }
  if (!strcmp(cmd, "verify") && argc == 6) {  // file n seed invert
    std::vector<uint32_t> buf(num(argv[3]));
    FILE* f = fopen(argv[2], "rb");
    if (!f || fread(buf.data(), 4, buf.size(), f) != buf.size()) return 3;
    fclose(f);
    const PatternReport r = host_verify(buf.data(), buf.size(), (uint32_t)num(argv[4]),
                                        (uint32_t)num(argv[5]));
    printf("%llu %llu %u %u\n", r.n_bad, r.first_bad, r.bits_bad, r.pad);
    return 0;
  }
  if (!strcmp(cmd, "plan") && argc == 4) {  // vram_bytes chunk_bytes (as the options)
    const Sizes s = normalise_sizes(atoll(argv[2]), 0, atoll(argv[3]));
    const ChunkPlan plan = chunk_plan(s.vram_words, s.chunk_words);
    unsigned long long sum = 0, biggest = 0, not_vectors = 0, bad_trips = 0, empty = 0;
    const unsigned long long count = plan.count();
    for (unsigned long long c = 0; c < count; ++c) {
      const unsigned long long n = plan.words(c);
      if (plan.base(c) != sum) ++bad_trips;  // a chunk starts where the last ended
      sum += n;
      if (n > biggest) biggest = n;
      if (n == 0) ++empty;
      if (c + 1 < count && n % 4) ++not_vectors;
      const ChunkPos first = locate(plan, plan.base(c));
      const ChunkPos last = locate(plan, plan.base(c) + n - 1);
      if (first.chunk != c || first.word != 0) ++bad_trips;
      if (last.chunk != c || last.word != n - 1) ++bad_trips;
    }
    const ChunkPos end = locate(plan, s.vram_words - 1);
    if (end.chunk != count - 1 || end.word != plan.words(count - 1) - 1) ++bad_trips;
    printf("%llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)s.vram_words,
           (unsigned long long)s.chunk_words, count, sum, biggest, not_vectors, bad_trips,
           empty);
    printf("%llu %llu\n", (unsigned long long)plan.words(0),
           (unsigned long long)plan.words(count - 1));
    return 0;
  }
  if (!strcmp(cmd, "locate") && argc == 5) {  // vram_bytes chunk_bytes span_word
    const Sizes s = normalise_sizes(atoll(argv[2]), 0, atoll(argv[3]));
    const ChunkPos pos = locate(chunk_plan(s.vram_words, s.chunk_words), num(argv[4]));
    printf("%llu %llu\n", (unsigned long long)pos.chunk, (unsigned long long)pos.word);
    return 0;
  }
  if (!strcmp(cmd, "sizes") && argc == 5) {  // vram_bytes link_bytes chunk_bytes
    const Sizes s = normalise_sizes(atoll(argv[2]), atoll(argv[3]), atoll(argv[4]));
    printf("%llu %llu %llu\n", (unsigned long long)s.vram_words,
           (unsigned long long)s.link_words, (unsigned long long)s.chunk_words);
    return 0;
  }
  if (!strcmp(cmd, "stages") && argc == 3) {  // seed
    for (int stage = 0; stage < kNumStages; ++stage)
      for (uint32_t pass = 0; pass < (stage == kVram ? 2u : 1u); ++pass) {
        const StagePattern p = stage_pattern(stage, pass, (uint32_t)num(argv[2]));
        printf("%s %u %u %u\n", kStages[stage].name, pass, p.seed, p.invert);
      }
    return 0;
  }
  return 2;
}
"""


@pytest.fixture(scope="module")
def integrity_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("integrity"), "integrity_main", INTEGRITY_MAIN)


def _run(exe, *args):
    return subprocess.run([exe, *map(str, args)], check=True, capture_output=True,
                          text=True).stdout


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_host_fill_matches_numpy(integrity_exe, n, invert):
    got = np.array([int(v) for v in _run(integrity_exe, "fill", n, SEED, invert).split()],
                   dtype=np.uint32)
    assert np.array_equal(got, probe_mod.pattern_words(0, n, SEED, invert))


def _verify_reference(words, seed, invert):
    """What a verify of ``words`` as span words 0.. must report, in numpy."""
    diff = words ^ probe_mod.pattern_words(0, words.size, seed, invert)
    bad = np.flatnonzero(diff)
    first = int(bad[0]) if bad.size else (1 << 64) - 1
    return [int(bad.size), first, int(np.bitwise_or.reduce(diff)), 0]


_HV_N = 1027
# the spread of tests/test_probe_integrity_gpu.py, folded into 1027 words
_HV_SPREAD = [5, 130, 131, 255, 256, 511, 512, 600, 700, 767, 768, 800, 900, 1000, 1023,
              1024, 1026]


def _host_verify_cases():
    clean = probe_mod.pattern_words(0, _HV_N, SEED, 0)
    cases = {"clean": (clean, SEED, 0), "clean inverted":
             (probe_mod.pattern_words(0, _HV_N, SEED, 1), SEED, 1)}
    for name, index, bit in (("first", 0, 0), ("middle", 513, 17), ("last", _HV_N - 1, 31)):
        words = clean.copy()
        words[index] ^= np.uint32(1 << bit)
        cases[f"one bit {name}"] = (words, SEED, 0)
    words = clean.copy()
    for k, i in enumerate(_HV_SPREAD):
        words[i] ^= np.uint32((1 << (k % 32)) | (1 << ((3 * k + 7) % 32)))
    cases["spread"] = (words, SEED, 0)
    cases["wrong seed"] = (clean, SEED ^ 1, 0)
    cases["wrong polarity"] = (clean, SEED, 1)
    return cases


HOST_VERIFY_CASES = _host_verify_cases()


@pytest.mark.parametrize("name", list(HOST_VERIFY_CASES))
def test_host_verify_matches_numpy(integrity_exe, tmp_path, name):
    words, seed, invert = HOST_VERIFY_CASES[name]
    path = tmp_path / "words.bin"
    words.tofile(path)
    got = [int(v) for v in _run(integrity_exe, "verify", path, words.size, seed, invert).split()]
    want = _verify_reference(words, seed, invert)
    assert got == want
    # the reference itself, where the answer is known in closed form
    if name.startswith("clean"):
        assert want == [0, (1 << 64) - 1, 0, 0]
    if name == "one bit last":
        assert want == [1, _HV_N - 1, 1 << 31, 0]
    if name == "spread":
        assert len(set(_HV_SPREAD)) == 17 and want[:2] == [17, 5]
    if name == "wrong seed":
        assert want[:2] == [_HV_N, 0]  # the mix is a bijection: every word differs
    if name == "wrong polarity":
        assert want == [_HV_N, 0, 0xFFFFFFFF, 0]


PLAN_VRAM = [4, 100, 3 * MIB + 20, 3 * MIB + 22, 1 << 30, (1 << 30) + 4, 3 * (1 << 30) + 20]
PLAN_CHUNK = [0, 5, 16, MIB, MIB + 7, 1 << 30, 1 << 31]


def _expected_chunk_words(chunk_bytes):
    """croprobe.h: 0 or more than 1 GiB is 1 GiB; whole 16-byte vectors, at least one."""
    if chunk_bytes <= 0 or chunk_bytes > 1 << 30:
        chunk_bytes = 1 << 30
    return max(chunk_bytes - chunk_bytes % 16, 16) // 4


@pytest.mark.parametrize("chunk_bytes", PLAN_CHUNK)
@pytest.mark.parametrize("vram_bytes", PLAN_VRAM)
def test_chunk_plan_and_locate(integrity_exe, vram_bytes, chunk_bytes):
    lines = _run(integrity_exe, "plan", vram_bytes, chunk_bytes).splitlines()
    (vram_words, chunk_words, count, total, biggest, not_vectors, bad_trips,
     empty) = (int(v) for v in lines[0].split())
    first, last = (int(v) for v in lines[1].split())
    want_chunk = _expected_chunk_words(chunk_bytes)
    want_count = -(-(vram_bytes // 4) // want_chunk)
    assert vram_words == vram_bytes >> 2 and chunk_words == want_chunk
    assert total == vram_bytes >> 2  # the counts sum to the span, whole words only
    assert not_vectors == 0  # every chunk but the last is a multiple of 4 words
    assert biggest <= 1 << 28 and empty == 0
    assert count == want_count
    assert bad_trips == 0  # bases are running sums; locate round-trips at every edge
    assert first == min(want_chunk, vram_words)
    assert last == vram_words - (want_count - 1) * want_chunk
    if (vram_bytes, chunk_bytes) == (100, 5):
        assert (count, first, last) == (7, 4, 1)  # six vectors and one tail word
    if (vram_bytes, chunk_bytes) in ((3 * MIB + 20, MIB + 7), (3 * MIB + 22, MIB)):
        assert (count, first, last) == (4, MIB // 4, 5)
    if (vram_bytes, chunk_bytes) == ((1 << 30) + 4, 0):
        assert (count, last) == (2, 1)  # a last chunk that is tail only


@pytest.mark.parametrize("word,want", [
    (0, (0, 0)), (MIB // 4 - 1, (0, MIB // 4 - 1)), (MIB // 4, (1, 0)),
    (2 * (MIB // 4), (2, 0)), (3 * (MIB // 4) - 1, (2, MIB // 4 - 1)),
    (3 * (MIB // 4), (3, 0)), (3 * (MIB // 4) + 4, (3, 4)),
])
def test_locate_known_words(integrity_exe, word, want):
    got = _run(integrity_exe, "locate", 3 * MIB + 20, MIB, word).split()
    assert (int(got[0]), int(got[1])) == want


def test_sizes_normalised(integrity_exe):
    def sizes(*args):
        return tuple(int(v) for v in _run(integrity_exe, "sizes", *args).split())

    assert sizes(0, 0, 0) == ((1 << 30) // 4, (256 * MIB) // 4, (1 << 30) // 4)
    assert sizes(-5, -5, -5) == sizes(0, 0, 0)
    assert sizes(7, 4, 15) == (1, 1, 4)
    assert sizes(3, 3, 16) == (0, 0, 4)  # below one word: the driver refuses
    assert sizes(3 * MIB + 22, MIB + 23, 31) == ((3 * MIB + 20) // 4, (MIB + 20) // 4, 4)


# The documented table (cro_amd/hip/integrity.hip, croprobe.h): VRAM holds the
# pattern and then its complement; the device→host stages run on
# seed ^ 0xA5A5A5A5; the shader stages hold the complement.
STAGE_PATTERNS = {
    ("vram", 0): (SEED, 0),
    ("vram", 1): (SEED, 1),
    ("h2d_dma", 0): (SEED, 0),
    ("d2h_dma", 0): (SEED_BACK, 0),
    ("h2d_kernel", 0): (SEED, 1),
    ("d2h_kernel", 0): (SEED_BACK, 1),
}


def test_stage_seed_and_polarity_table(integrity_exe):
    got = {}
    order = []
    for line in _run(integrity_exe, "stages", SEED).splitlines():
        name, stage_pass, seed, invert = line.split()
        got[(name, int(stage_pass))] = (int(seed), int(invert))
        if name not in order:
            order.append(name)
    assert got == STAGE_PATTERNS
    assert tuple(order) == probe_mod.INTEGRITY_STAGES  # selftest_stage - 1 indexes both


def test_guard_preset_differs_from_pattern_at_every_slack_index():
    """The raw entries preset the 0-3 slack words after n_words to 0xA5 bytes;
    a verify that read one word too many sees a mismatch only if that is not
    what the pattern holds there.  It is not, for any shape the GPU tests use."""
    from tests.test_probe_integrity_gpu import SEED as GPU_SEED, SHAPES

    checked = 0
    for base, n in SHAPES:
        slack = -n % 4
        for invert in (0, 1):
            words = probe_mod.pattern_words(base + n, slack, GPU_SEED, invert)
            assert not np.any(words == np.uint32(0xA5A5A5A5)), (base, n, invert)
            checked += slack
    assert checked > 0


# -- structs --------------------------------------------------------------------


def _struct_main():
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "croprobe.h"', "int main() {"]
    for cname, mirror in (
        ("CroIntegrityOpts", probe_mod.CroIntegrityOpts),
        ("CroIntegrityResult", probe_mod.CroIntegrityResult),
    ):
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for field, _ in mirror._fields_:
            lines.append(
                f'  printf("{cname} {field} %zu %zu\\n", offsetof({cname}, {field}), '
                f"sizeof((({cname}*)0)->{field}));"
            )
    lines += ["  return 0;", "}"]
    return "\n".join(lines)


def test_struct_layout_matches_ctypes(tmp_path):
    """Every field the ctypes mirrors name exists in the header at the same
    offset and size, and the totals agree (so the header has no extra one)."""
    opts_fields = [f for f, _ in probe_mod.CroIntegrityOpts._fields_]
    assert opts_fields[4:] == ["selftest_stage", "link_floor_gbps", "selftest_pass",
                               "selftest_bit", "selftest_word"]
    assert [f for f, _ in probe_mod.CroIntegrityResult._fields_][-2:] == ["first_bad_got",
                                                                         "reserved"]
    exe = _build(tmp_path, "struct_main", _struct_main())
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    mirrors = {
        "CroIntegrityOpts": probe_mod.CroIntegrityOpts,
        "CroIntegrityResult": probe_mod.CroIntegrityResult,
    }
    seen = 0
    for line in out.splitlines():
        parts = line.split()
        mirror = mirrors[parts[0]]
        if parts[1] == "sizeof":
            assert ctypes.sizeof(mirror) == int(parts[2]), line
        else:
            desc = getattr(mirror, parts[1])
            assert (desc.offset, desc.size) == (int(parts[2]), int(parts[3])), line
        seen += 1
    assert seen == 2 + sum(len(m._fields_) for m in mirrors.values())
    # no padding holes a renamed or dropped header field could hide in
    for mirror in mirrors.values():
        end = 0
        for field, _ in mirror._fields_:
            desc = getattr(mirror, field)
            assert desc.offset == end, (mirror.__name__, field)
            end = desc.offset + desc.size
        assert end == ctypes.sizeof(mirror)


# -- make_probe_fn ----------------------------------------------------------------


class Gpu:
    pci_bdf = "0000:05:00.0"


def _patch_probe(monkeypatch, quick, integrity):
    calls = {"quick": [], "integrity": []}

    def run_probe(device=0):
        calls["quick"].append(device)
        return dict(quick)

    def run_integrity(device=0, **kw):
        calls["integrity"].append((device, kw))
        return dict(integrity)

    monkeypatch.setattr(probe_mod, "hip_device_for_bdf", lambda bdf: 3)
    monkeypatch.setattr(probe_mod, "run_probe", run_probe)
    monkeypatch.setattr(probe_mod, "run_integrity", run_integrity)
    return calls


BAD_INTEGRITY = {
    "ok": False, "rc": -20, "n_bad": 3, "first_bad_byte": 4096, "bits_bad": 0x10,
    "failed_stage": "vram", "msg": "data mismatch in stage vram",
}
GOOD_INTEGRITY = {
    "ok": True, "rc": 0, "n_bad": 0, "failed_stage": "", "msg": "ok",
    "vram_passes": 2, "vram_bytes_verified": 2 << 30,
    "h2d_dma_bytes_verified": 256 << 20, "d2h_dma_bytes_verified": 256 << 20,
    "h2d_dma_gbps": 51.5, "d2h_dma_gbps": 49.0,
}
GOOD_QUICK = {"ok": True, "rc": 0, "mfma_f32_exact": True, "hbm_gbps": 4000.0, "msg": "ok"}


def test_make_probe_fn_quick_is_todays_hook():
    assert probe_mod.make_probe_fn("quick") is probe_mod.probe_fn_for_nodeops
    with pytest.raises(ValueError):
        probe_mod.make_probe_fn("thorough")


def test_deep_stops_after_failed_quick(monkeypatch):
    calls = _patch_probe(monkeypatch, {"ok": False, "rc": -2, "msg": "mfma"}, GOOD_INTEGRITY)
    result = probe_mod.make_probe_fn("deep")(Gpu())
    assert result["ok"] is False and "integrity" not in result
    assert calls["quick"] == [3] and calls["integrity"] == []


def test_deep_bad_integrity_fails_and_keeps_result(monkeypatch):
    calls = _patch_probe(monkeypatch, GOOD_QUICK, BAD_INTEGRITY)
    fn = probe_mod.make_probe_fn("deep", vram_bytes=64 << 20, link_bytes=16 << 20,
                                 link_floor_gbps=5.0)
    result = fn(Gpu())
    assert result["ok"] is False
    assert result["integrity"] == BAD_INTEGRITY
    assert result["mfma_f32_exact"] is True  # quick fields kept
    device, kw = calls["integrity"][0]
    assert device == 3  # same ordinal as the quick probe
    assert kw["vram_bytes"] == 64 << 20 and kw["link_bytes"] == 16 << 20
    assert kw["link_floor_gbps"] == 5.0


def test_deep_both_ok(monkeypatch):
    _patch_probe(monkeypatch, GOOD_QUICK, GOOD_INTEGRITY)
    result = probe_mod.make_probe_fn("deep")(Gpu())
    assert result["ok"] is True and result["integrity"] == GOOD_INTEGRITY


# -- probe_via_exec ---------------------------------------------------------------


class RecordingExec:
    def __init__(self, out='{"ok": true}'):
        self.argvs = []
        self.out = out

    def run(self, node, argv, timeout=None):
        self.argvs.append(list(argv))
        return 0, self.out, ""


def test_exec_probe_quick_argv_unchanged():
    ex = RecordingExec()
    probe_mod.probe_via_exec(ex, "n0", Gpu())
    probe_mod.make_exec_probe_fn(ex, "n0", argv_prefix_fn=lambda: ["chroot", "/d"])(Gpu())
    assert ex.argvs == [
        ["croagent", "probe", "--bdf", "0000:05:00.0"],
        ["chroot", "/d", "croagent", "probe", "--bdf", "0000:05:00.0"],
    ]


def test_exec_probe_deep_argv():
    ex = RecordingExec('{"ok": true, "integrity": {"ok": true}}')
    out = probe_mod.probe_via_exec(ex, "n0", Gpu(), level="deep", vram_mib=64, link_mib=16,
                                   link_floor_gbps=12.5)
    assert out["integrity"]["ok"] is True
    probe_mod.make_exec_probe_fn(ex, "n0", level="deep")(Gpu())
    assert ex.argvs == [
        ["croagent", "probe", "--bdf", "0000:05:00.0", "--deep", "--vram-mib", "64",
         "--link-mib", "16", "--link-floor-gbps", "12.5"],
        ["croagent", "probe", "--bdf", "0000:05:00.0", "--deep"],
    ]
    with pytest.raises(ValueError):
        probe_mod.make_exec_probe_fn(ex, "n0", level="thorough")


# -- controller -------------------------------------------------------------------


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


def test_controller_refuses_online_on_integrity_failure(mock_world):
    probe = dict(GOOD_QUICK, ok=False, integrity=BAD_INTEGRITY)
    _attach(mock_world, probe)
    counter = mock_world.resource_rec.metrics.probe_integrity_failures_total.labels(stage="vram")
    before = counter._value.get()
    with pytest.raises(FabricError):
        mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Attaching"
    assert "health probe failed" in got.status.error
    assert "stage vram" in got.status.error
    assert "first_bad_byte=4096" in got.status.error
    assert "bits_bad=0x00000010" in got.status.error
    assert counter._value.get() == before + 1


def test_controller_online_event_carries_integrity_summary(mock_world):
    _attach(mock_world, dict(GOOD_QUICK, integrity=GOOD_INTEGRITY))
    mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Online"
    message = _online_message(mock_world)
    assert "integrity: vram 1.00 GiB link 0.25 GiB verified" in message
    assert "h2d 51.5 d2h 49.0 GB/s" in message


def test_controller_online_event_unchanged_without_integrity(mock_world):
    _attach(mock_world, dict(GOOD_QUICK))
    mock_world.resource_rec.reconcile("gpu-1")
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Online"
    assert _online_message(mock_world) == (
        f"device {got.status.device_id} online with CDI spec"
        "; probe: mfma_exact=True hbm=4000 GB/s"
    )


def test_metrics_reset_unregisters_integrity_counter():
    from prometheus_client import REGISTRY

    from cro_amd.metrics import Metrics

    Metrics()
    assert "cro_probe_integrity_failures" in REGISTRY._names_to_collectors
    Metrics._reset_for_tests()
    try:
        assert "cro_probe_integrity_failures" not in REGISTRY._names_to_collectors
    finally:
        Metrics()  # later tests share the process-wide singleton


# -- entrypoint -------------------------------------------------------------------


def _parse(argv):
    from cro_amd.cmd.main import add_probe_arguments

    p = argparse.ArgumentParser()
    add_probe_arguments(p)
    return p.parse_args(argv)


def test_entrypoint_default_is_quick(monkeypatch):
    from cro_amd.cmd.main import select_probe_fn

    monkeypatch.delenv("CRO_PROBE_LEVEL", raising=False)
    args = _parse([])
    assert args.probe_level == "quick"
    assert select_probe_fn(args) is probe_mod.probe_fn_for_nodeops


def test_entrypoint_flag_selects_deep(monkeypatch):
    from cro_amd.cmd.main import select_probe_fn

    monkeypatch.delenv("CRO_PROBE_LEVEL", raising=False)
    args = _parse(["--probe-level", "deep", "--probe-vram-mib", "64", "--probe-link-mib", "16",
                   "--probe-link-floor-gbps", "7.5"])
    fn = select_probe_fn(args)
    assert fn is not probe_mod.probe_fn_for_nodeops and fn.level == "deep"
    calls = _patch_probe(monkeypatch, GOOD_QUICK, GOOD_INTEGRITY)
    assert fn(Gpu())["integrity"] == GOOD_INTEGRITY
    _, kw = calls["integrity"][0]
    assert kw["vram_bytes"] == 64 << 20 and kw["link_bytes"] == 16 << 20
    assert kw["link_floor_gbps"] == 7.5


def test_entrypoint_env_selects_deep(monkeypatch):
    from cro_amd.cmd.main import select_probe_fn

    monkeypatch.setenv("CRO_PROBE_LEVEL", "deep")
    assert select_probe_fn(_parse([])).level == "deep"
    # the flag wins over the environment
    assert select_probe_fn(_parse(["--probe-level", "quick"])) is probe_mod.probe_fn_for_nodeops


# -- build --------------------------------------------------------------------


def test_build_rebuilds_when_any_source_or_header_is_newer(tmp_path):
    from cro_amd.hip import build as hip_build

    names = {os.path.basename(p) for p in hip_build.SRCS + hip_build.HEADERS}
    assert names == {"probe.hip", "integrity.hip", "croprobe.h", "cropattern.h"}
    assert all(os.path.exists(p) for p in hip_build.SRCS + hip_build.HEADERS)
    out, src, hdr = tmp_path / "lib.so", tmp_path / "a.hip", tmp_path / "a.h"
    for path in (src, hdr):
        path.write_text("")
    assert hip_build._stale(str(out), [str(src), str(hdr)])  # missing output
    out.write_text("")
    os.utime(src, (100, 100))
    os.utime(hdr, (100, 100))
    os.utime(out, (200, 200))
    assert not hip_build._stale(str(out), [str(src), str(hdr)])
    os.utime(hdr, (300, 300))
    assert hip_build._stale(str(out), [str(src), str(hdr)])
