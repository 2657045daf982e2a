"""CPU tests of the LDS scrub stage: the two C structs against their Python
mirrors and the record aggregation (through small host programs built with the
host C++ compiler — no HIP, no GPU), the library loader, the operator flags,
the merge of the VRAM and LDS results, the exec path, the controller's scrub
phase with an LDS result, the agent's ``scrub --lds`` on a machine without a
GPU, and the build of the library."""

import argparse
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest

from cro_amd.api.v1alpha1.types import ComposableResource, Event
from cro_amd.nodeops import ldsscrub as lds_mod
from cro_amd.nodeops import scrub as scrub_mod
from cro_amd.nodeops.amdgpu import ScrubFailed
from tests.conftest import make_node, make_resource

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(REPO, "cro_amd", "hip")
AGENT = os.path.join(REPO, "cro_amd", "agent", "croagent")
MIB = 1 << 20
GIB = 1 << 30
NONE64 = (1 << 64) - 1
LDS = 163840


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


# -- struct mirrors ----------------------------------------------------------------

MIRRORS = {"CroLdsScrubOpts": lds_mod.CroLdsScrubOpts,
           "CroLdsScrubResult": lds_mod.CroLdsScrubResult}


def _layout_source():
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "croldsscrub.h"',
             "int main() {"]
    for cname, mirror in MIRRORS.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for field, _ in mirror._fields_:
            lines.append(
                f'  printf("{cname} {field} %zu %zu\\n", offsetof({cname}, {field}), '
                f"sizeof((({cname}*)0)->{field}));"
            )
    lines += ['  printf("record sizeof %zu\\n", sizeof(CroLdsScrubRecord));',
              '  printf("consts %d %d %u\\n", (int)CRO_LDS_SCRUB_BYTES, (int)CRO_LDS_SCRUB_WORDS, '
              "CRO_LDS_SCRUB_GUARD_WORD);",
              "  return 0;", "}"]
    return "\n".join(lines)


def test_struct_mirrors_match_the_header(tmp_path):
    exe = _build(tmp_path, "lds_layout", _layout_source())
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    seen = set()
    for line in out.splitlines():
        parts = line.split()
        if parts[0] == "record":
            assert int(parts[2]) == 40  # ten 32-bit words, what the kernel's atomics index
            continue
        if parts[0] == "consts":
            assert [int(v) for v in parts[1:]] == [LDS, LDS // 4, lds_mod.GUARD_WORD]
            assert lds_mod.LDS_BYTES == LDS
            continue
        mirror = MIRRORS[parts[0]]
        if parts[1] == "sizeof":
            assert ctypes.sizeof(mirror) == int(parts[2]), line
        else:
            desc = getattr(mirror, parts[1])
            assert (desc.offset, desc.size) == (int(parts[2]), int(parts[3])), line
        seen.add((parts[0], parts[1]))
    assert len(seen) == sum(len(m._fields_) + 1 for m in MIRRORS.values())


def test_struct_mirrors_have_no_holes():
    """A hole would be a field of the header that the mirror lacks."""
    for mirror in MIRRORS.values():
        end = 0
        for field, _ in mirror._fields_:
            desc = getattr(mirror, field)
            assert desc.offset == end, (mirror.__name__, field)
            end = desc.offset + desc.size
        assert end == ctypes.sizeof(mirror)


def test_result_has_the_fields_the_operator_reads():
    names = [f for f, _ in lds_mod.CroLdsScrubResult._fields_]
    for want in ("ok", "rc", "cus_expected", "cus_seen", "xcds_seen", "workgroups", "rounds",
                 "lds_bytes", "bytes_scrubbed", "dirty_words_before", "dirty_workgroups",
                 "first_dirty_word", "n_bad", "first_bad_word", "bits_bad", "guard_bad",
                 "recheck_dirty_words", "xcd", "se", "sh", "cu", "gpu_ms", "t_total_ms", "msg"):
        assert want in names, want
    assert names[:2] == ["ok", "rc"]
    assert lds_mod.CroLdsScrubResult.msg.size == 256


# -- croldsscrub.h aggregation -------------------------------------------------------

AGG_MAIN = r"""
#include <cstdio>
#include <vector>
#include "croldsscrub.h"

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("line %d: %s\n", __LINE__, #cond);                   \
      return 1;                                                   \
    }                                                             \
  } while (0)

static CroLdsScrubRecord rec(unsigned xcd, unsigned se, unsigned sh, unsigned cu, unsigned simd,
                             unsigned wave) {
  CroLdsScrubRecord r = CRO_LDS_SCRUB_CLEAN_RECORD;
  r.xcc_id = xcd | 0xABC0u;  // bits above 3:0 are not the XCD
  r.hw_id = (se << 13) | (sh << 12) | (cu << 8) | (simd << 4) | wave | 0x40u;  // and PIPE_ID
  r.valid = 1;
  return r;
}

int main() {
  CroLdsScrubAgg a;
  // no records
  cro_lds_scrub_aggregate(nullptr, 0, &a);
  EXPECT(a.workgroups == 0 && a.cus_seen == 0 && a.xcds_seen == 0);
  EXPECT(a.dirty_words == 0 && a.dirty_workgroups == 0 && a.n_bad == 0 && a.guard_bad == 0);
  EXPECT(a.bad_workgroups == 0 && a.bits_bad == 0);
  EXPECT(a.first_bad_index == -1 && a.xcd == -1 && a.se == -1 && a.sh == -1 && a.cu == -1);
  EXPECT(a.first_dirty_word == ~0u && a.first_bad_word == ~0u);

  // the clean record is what the host presets
  const CroLdsScrubRecord clean = CRO_LDS_SCRUB_CLEAN_RECORD;
  EXPECT(clean.valid == 0 && clean.first_dirty == ~0u && clean.first_bad == ~0u);
  EXPECT(clean.dirty_words == 0 && clean.n_bad == 0 && clean.bits_bad == 0);

  // invalid records are skipped, whatever they hold
  std::vector<CroLdsScrubRecord> v(3, clean);
  v[1].n_bad = 9;
  v[1].first_bad = 1;
  v[1].dirty_words = 5;
  v[1].guard_bad = 2;
  cro_lds_scrub_aggregate(v.data(), v.size(), &a);
  EXPECT(a.workgroups == 0 && a.n_bad == 0 && a.dirty_words == 0 && a.guard_bad == 0);
  EXPECT(a.first_bad_index == -1 && a.cus_seen == 0);

  // sums, distinct CU keys, first bad by lowest index and its decoded location
  v.clear();
  v.push_back(rec(0, 0, 0, 0, 0, 0));    // 0
  v.push_back(rec(0, 0, 0, 0, 3, 7));    // 1: the same CU on another SIMD and wave slot
  v.push_back(clean);                    // 2: invalid
  v.push_back(rec(7, 3, 1, 15, 1, 2));   // 3: bad
  v.push_back(rec(7, 3, 1, 14, 0, 0));   // 4: bad, lower word, later index
  v.push_back(rec(1, 0, 0, 0, 0, 0));    // 5: another XCD, same SE/SH/CU as record 0
  v.push_back(rec(0, 0, 1, 0, 0, 0));    // 6: another SH
  v[0].dirty_words = 40960;
  v[0].first_dirty = 0;
  v[1].dirty_words = 3;
  v[1].first_dirty = 17;
  v[3].n_bad = 2;
  v[3].first_bad = 1024;
  v[3].bits_bad = 0x80000000u;
  v[3].guard_bad = 4;
  v[4].n_bad = 5;
  v[4].first_bad = 3;
  v[4].bits_bad = 0x00000001u;
  v[5].dirty_words = 1;
  v[5].first_dirty = 40959;
  v[6].guard_bad = 1;
  cro_lds_scrub_aggregate(v.data(), v.size(), &a);
  EXPECT(a.workgroups == 6);
  EXPECT(a.cus_seen == 5 && a.xcds_seen == 3);
  EXPECT(a.dirty_words == 40964 && a.dirty_workgroups == 3 && a.first_dirty_word == 0);
  EXPECT(a.n_bad == 7 && a.guard_bad == 5 && a.bad_workgroups == 3);
  EXPECT(a.bits_bad == 0x80000001u);
  EXPECT(a.first_bad_index == 3 && a.first_bad_word == 1024);
  EXPECT(a.xcd == 7 && a.se == 3 && a.sh == 1 && a.cu == 15);
  const CroCoverageLoc loc = cro_cov_decode(v[3].xcc_id, v[3].hw_id);
  EXPECT((int)loc.xcd == a.xcd && (int)loc.se == a.se && (int)loc.sh == a.sh &&
         (int)loc.cu == a.cu);

  // a prefix: one pass in record order gives the prefix's own answer
  cro_lds_scrub_aggregate(v.data(), 3, &a);
  EXPECT(a.workgroups == 2 && a.cus_seen == 1 && a.xcds_seen == 1);
  EXPECT(a.dirty_words == 40963 && a.first_dirty_word == 0 && a.first_bad_index == -1);
  // the lowest dirty offset is a minimum, not the first
  cro_lds_scrub_aggregate(v.data() + 1, 5, &a);
  EXPECT(a.first_dirty_word == 17 && a.dirty_words == 4 && a.first_bad_index == 2);

  // every CU of an MI355X: 8 XCDs x 4 SEs x 8 CUs, twice over
  v.clear();
  for (int round = 0; round < 2; ++round)
    for (unsigned xcd = 0; xcd < 8; ++xcd)
      for (unsigned se = 0; se < 4; ++se)
        for (unsigned cu = 0; cu < 8; ++cu) v.push_back(rec(xcd, se, 0, cu, round, round));
  cro_lds_scrub_aggregate(v.data(), v.size(), &a);
  EXPECT(a.workgroups == 512 && a.cus_seen == 256 && a.xcds_seen == 8);
  // the largest fields the decode has
  v.assign(1, rec(15, 7, 1, 15, 3, 15));
  v[0].n_bad = 1;
  v[0].first_bad = 40959;
  cro_lds_scrub_aggregate(v.data(), 1, &a);
  EXPECT(a.cus_seen == 1 && a.xcd == 15 && a.se == 7 && a.sh == 1 && a.cu == 15);
  printf("ok\n");
  return 0;
}
"""


def test_aggregation_exact_cases(tmp_path):
    exe = _build(tmp_path, "ldsagg_main", AGG_MAIN)
    proc = subprocess.run([exe], capture_output=True, text=True)
    assert proc.returncode == 0 and proc.stdout.strip() == "ok", proc.stdout + proc.stderr


def test_aggregation_program_under_host_sanitizers(tmp_path):
    """The same stand-alone host program, built with ASan and UBSan."""
    try:
        exe = _build(tmp_path, "ldsagg_san", AGG_MAIN,
                     extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    except subprocess.CalledProcessError as exc:
        pytest.skip(f"host compiler cannot build with sanitizers: {exc.stderr[-200:]}")
    proc = subprocess.run([exe], capture_output=True, text=True)
    assert proc.returncode == 0 and proc.stdout.strip() == "ok", proc.stdout + proc.stderr
    assert "runtime error" not in proc.stderr and "Sanitizer" not in proc.stderr


# -- library loading -----------------------------------------------------------------


def test_load_lds_scrub_library_is_loud_only_where_required(monkeypatch, tmp_path):
    monkeypatch.setattr(lds_mod, "_lib", None)
    monkeypatch.setattr(lds_mod, "_LIB_PATH", str(tmp_path / "libcroldsscrub.so"))
    assert lds_mod.load_lds_scrub_library(required=False) is None
    with pytest.raises(RuntimeError, match="libcroldsscrub.so missing"):
        lds_mod.load_lds_scrub_library(required=True)
    monkeypatch.setattr(lds_mod, "_gpu_present", lambda: True)
    with pytest.raises(RuntimeError, match="on a GPU node"):
        lds_mod.load_lds_scrub_library()
    monkeypatch.setattr(lds_mod, "_gpu_present", lambda: False)
    assert lds_mod.load_lds_scrub_library() is None
    # run_lds_scrub always requires it
    with pytest.raises(RuntimeError, match="libcroldsscrub.so missing"):
        lds_mod.run_lds_scrub(0)


def test_opts_take_the_keywords_of_the_struct():
    o = lds_mod._lds_scrub_opts(lds_bytes=16, grid=2, max_rounds=1, skip_recheck=1,
                                fill_word=-1, min_cu_fraction=0.5, selftest_mode=4,
                                selftest_pattern=0x1_0000_0001, selftest_word=3, selftest_bit=31)
    assert (o.lds_bytes, o.grid, o.max_rounds, o.skip_recheck, o.fill_word) == (
        16, 2, 1, 1, 0xFFFFFFFF)
    assert (o.min_cu_fraction, o.selftest_mode, o.selftest_pattern, o.selftest_word,
            o.selftest_bit, o.reserved) == (0.5, 4, 1, 3, 31, 0)
    with pytest.raises(TypeError):
        lds_mod._lds_scrub_opts(no_such_option=1)


# -- entry point ---------------------------------------------------------------------

SCRUB_ENV = ("CRO_SCRUB_ON_DETACH", "CRO_SCRUB_MAX_MIB", "CRO_SCRUB_RESERVE_MIB",
             "CRO_SCRUB_MIN_FRACTION", "CRO_SCRUB_LDS", "CRO_SCRUB_LDS_MIN_CU_FRACTION")


def _parser(monkeypatch, env=None):
    from cro_amd.cmd.main import add_scrub_arguments

    for name in SCRUB_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    p = argparse.ArgumentParser()
    add_scrub_arguments(p)
    return p


def _parse(argv, monkeypatch, env=None):
    return _parser(monkeypatch, env).parse_args(argv)


def test_lds_flags_default_off(monkeypatch):
    args = _parse([], monkeypatch)
    assert (args.scrub_lds, args.scrub_lds_min_cu_fraction) == ("off", 0.0)


def test_lds_flags_and_environment(monkeypatch):
    args = _parse(["--scrub-on-detach", "on", "--scrub-lds", "on",
                   "--scrub-lds-min-cu-fraction", "0.75"], monkeypatch)
    assert (args.scrub_lds, args.scrub_lds_min_cu_fraction) == ("on", 0.75)
    env = {"CRO_SCRUB_ON_DETACH": "on", "CRO_SCRUB_LDS": "on",
           "CRO_SCRUB_LDS_MIN_CU_FRACTION": "0.5"}
    args = _parse([], monkeypatch, env)
    assert (args.scrub_on_detach, args.scrub_lds, args.scrub_lds_min_cu_fraction) == (
        "on", "on", 0.5)
    # the flag wins over the environment
    args = _parse(["--scrub-lds", "off", "--scrub-lds-min-cu-fraction", "1"], monkeypatch, env)
    assert (args.scrub_lds, args.scrub_lds_min_cu_fraction) == ("off", 1.0)
    with pytest.raises(SystemExit):
        _parse(["--scrub-lds", "maybe"], monkeypatch)


def test_select_scrub_fn_keywords(monkeypatch):
    from cro_amd.cmd import main as main_mod

    made = []
    monkeypatch.setattr(scrub_mod, "make_scrub_fn", lambda **kw: made.append(kw) or "hook")
    argv = ["--scrub-on-detach", "on", "--scrub-max-mib", "3", "--scrub-min-fraction", "0.25"]
    # LDS off: today's three keywords exactly, whatever the LDS floor says
    for extra in ([], ["--scrub-lds", "off"], ["--scrub-lds-min-cu-fraction", "0.9"]):
        made.clear()
        assert main_mod.select_scrub_fn(_parse(argv + extra, monkeypatch)) == "hook"
        assert made == [{"max_bytes": 3 * MIB, "reserve_bytes": 0, "min_fraction": 0.25}]
    made.clear()
    args = _parse(argv + ["--scrub-lds", "on", "--scrub-lds-min-cu-fraction", "0.9"], monkeypatch)
    assert main_mod.select_scrub_fn(args) == "hook"
    assert made == [{"max_bytes": 3 * MIB, "reserve_bytes": 0, "min_fraction": 0.25,
                     "lds": True, "lds_min_cu_fraction": 0.9}]
    # the scrub off: no hook at all
    made.clear()
    assert main_mod.select_scrub_fn(_parse(["--scrub-lds", "on"], monkeypatch)) is None
    assert made == []


def test_lds_on_with_the_scrub_off_is_a_start_up_error(monkeypatch, capsys):
    from cro_amd.cmd import main as main_mod

    p = _parser(monkeypatch)
    with pytest.raises(SystemExit) as exc:
        main_mod.check_scrub_arguments(p, p.parse_args(["--scrub-lds", "on"]))
    assert exc.value.code == 2
    assert "--scrub-lds on needs --scrub-on-detach on" in capsys.readouterr().err
    for argv in ([], ["--scrub-on-detach", "on"], ["--scrub-on-detach", "on", "--scrub-lds", "on"]):
        main_mod.check_scrub_arguments(p, p.parse_args(argv))
    # and the operator's own entry refuses to start
    for name in SCRUB_ENV:
        monkeypatch.delenv(name, raising=False)
    with pytest.raises(SystemExit) as exc:
        main_mod.main(["--scrub-lds", "on"])
    assert exc.value.code == 2
    monkeypatch.setenv("CRO_SCRUB_LDS", "on")
    with pytest.raises(SystemExit) as exc:
        main_mod.main([])
    assert exc.value.code == 2


# -- merge of the two results ----------------------------------------------------------

VRAM_OK = {"ok": True, "rc": 0, "bytes_scrubbed": 64 * MIB, "n_bad": 0, "bits_bad": 0,
           "t_total_ms": 41.6, "msg": "ok"}
VRAM_BAD = dict(VRAM_OK, ok=False, rc=-40, n_bad=3, msg="residue after scrub: 3 bad words")
LDS_OK = {"ok": True, "rc": 0, "cus_expected": 256, "cus_seen": 256, "bytes_scrubbed": 256 * LDS,
          "dirty_words_before": 77, "n_bad": 0, "recheck_dirty_words": 0, "msg": "ok"}
LDS_BAD = dict(LDS_OK, ok=False, rc=-42, n_bad=2, first_bad_word=1024, bits_bad=0x10,
               xcd=3, se=1, sh=0, cu=5, msg="LDS residue at xcd=3 se=1 sh=0 cu=5")
LDS_LOW = dict(LDS_OK, ok=False, rc=-43, cus_seen=200, msg="LDS scrub reached 200 of 256 CUs")


class _Gpu:
    pci_bdf = "0000:5a:00.0"


@pytest.mark.parametrize("vram,lds,ok,rc,msg", [
    (VRAM_OK, LDS_OK, True, 0, "ok"),
    (VRAM_BAD, LDS_OK, False, -40, VRAM_BAD["msg"]),
    (VRAM_OK, LDS_BAD, False, -42, LDS_BAD["msg"]),
    (VRAM_OK, LDS_LOW, False, -43, LDS_LOW["msg"]),
    (VRAM_BAD, LDS_BAD, False, -40, VRAM_BAD["msg"]),  # the VRAM scrub's failure leads
])
def test_make_scrub_fn_merges_the_lds_result(monkeypatch, vram, lds, ok, rc, msg):
    calls = []
    monkeypatch.setattr(scrub_mod, "hip_device_for_bdf", lambda bdf: 3)
    monkeypatch.setattr(scrub_mod, "run_scrub",
                        lambda dev, **kw: calls.append(("vram", dev, kw)) or dict(vram))
    monkeypatch.setattr(lds_mod, "run_lds_scrub",
                        lambda dev, **kw: calls.append(("lds", dev, kw)) or dict(lds))
    fn = scrub_mod.make_scrub_fn(max_bytes=5, reserve_bytes=6, min_fraction=0.5, lds=True,
                                 lds_min_cu_fraction=0.9)
    got = fn(_Gpu())
    # the VRAM scrub first, then the LDS scrub, both on the device's ordinal
    assert calls == [("vram", 3, {"max_bytes": 5, "reserve_bytes": 6, "min_fraction": 0.5}),
                     ("lds", 3, {"min_cu_fraction": 0.9})]
    assert (got["ok"], got["rc"], got["msg"]) == (ok, rc, msg)
    assert got["lds"] == lds
    # everything else is the VRAM scrub's, in its order, with "lds" last
    assert list(got) == list(vram) + ["lds"]
    assert {k: v for k, v in got.items() if k not in ("ok", "rc", "msg", "lds")} == {
        k: v for k, v in vram.items() if k not in ("ok", "rc", "msg")}


def test_make_scrub_fn_without_lds_is_unchanged(monkeypatch):
    calls = []
    monkeypatch.setattr(scrub_mod, "hip_device_for_bdf", lambda bdf: None)
    monkeypatch.setattr(scrub_mod, "run_scrub",
                        lambda dev, **kw: calls.append((dev, kw)) or dict(VRAM_OK))

    def never(dev, **kw):
        raise AssertionError("the LDS scrub ran with lds off")

    monkeypatch.setattr(lds_mod, "run_lds_scrub", never)
    for fn in (scrub_mod.make_scrub_fn(), scrub_mod.make_scrub_fn(lds=False,
                                                                 lds_min_cu_fraction=0.9)):
        assert fn(_Gpu()) == VRAM_OK
    assert calls == [(0, {"max_bytes": 0, "reserve_bytes": 0, "min_fraction": 0.0})] * 2


# -- exec path -----------------------------------------------------------------------


class _Exec:
    def __init__(self, rc=0, out="", err=""):
        self.answer, self.calls = (rc, out, err), []

    def run(self, node, argv, timeout=None):
        self.calls.append((node, list(argv), timeout))
        return self.answer


def test_scrub_via_exec_argv_with_and_without_lds():
    merged = dict(VRAM_OK, lds=LDS_OK)
    base = ["croagent", "scrub", "--bdf", "0000:5a:00.0"]
    execer = _Exec(0, json.dumps(merged) + "\n")
    assert scrub_mod.scrub_via_exec(execer, "node7", _Gpu(), lds=True) == merged
    assert execer.calls == [("node7", base + ["--lds"], 300)]
    execer = _Exec(0, json.dumps(merged))
    scrub_mod.scrub_via_exec(execer, "node7", _Gpu(), argv_prefix=["chroot", "/x"], max_mib=64,
                             min_fraction=0.9, lds=True, lds_min_cu_fraction=0.75)
    assert execer.calls[0][1] == ["chroot", "/x"] + base + [
        "--max-mib", "64", "--min-fraction", "0.9", "--lds", "--lds-min-cu-fraction", "0.75"]
    # without lds: today's argv, and the floor alone adds nothing
    for kw in ({}, {"lds": False}, {"lds_min_cu_fraction": 0.75}):
        execer = _Exec(0, json.dumps(VRAM_OK))
        assert scrub_mod.scrub_via_exec(execer, "node7", _Gpu(), max_mib=64, **kw) == VRAM_OK
        assert execer.calls == [("node7", base + ["--max-mib", "64"], 300)]
    # the hook
    execer = _Exec(0, json.dumps(merged))
    scrub_mod.make_exec_scrub_fn(execer, "node7", max_mib=8, lds=True,
                                 lds_min_cu_fraction=1.0)(_Gpu())
    scrub_mod.make_exec_scrub_fn(execer, "node7", max_mib=8)(_Gpu())
    assert [c[1] for c in execer.calls] == [
        base + ["--max-mib", "8", "--lds", "--lds-min-cu-fraction", "1.0"],
        base + ["--max-mib", "8"]]


def test_scrub_via_exec_passes_lds_error_shapes_through():
    failed = dict(VRAM_OK, ok=False, rc=-42, msg=LDS_BAD["msg"], lds=LDS_BAD)
    assert scrub_mod.scrub_via_exec(_Exec(1, json.dumps(failed)), "n", _Gpu(), lds=True) == failed
    missing = {"ok": False, "rc": -1, "msg": "libcroldsscrub.so not available: no such file"}
    assert scrub_mod.scrub_via_exec(_Exec(1, json.dumps(missing)), "n", _Gpu(),
                                    lds=True) == missing
    assert scrub_mod.scrub_via_exec(_Exec(127, "", "croagent: not found\n"), "n", _Gpu(),
                                    lds=True) == {
        "ok": False, "rc": 127, "msg": "croagent: not found"}
    assert scrub_mod.scrub_via_exec(_Exec(0, "", ""), "n", _Gpu(), lds=True)["ok"] is False
    got = scrub_mod.scrub_via_exec(_Exec(0, "Segmentation fault", ""), "n", _Gpu(), lds=True)
    assert got == {"ok": False, "rc": 0, "msg": "unparseable scrub output: Segmentation fault"}


# -- controller ----------------------------------------------------------------------

OK_RESULT = {
    "ok": True, "rc": 0, "vram_total": 288 * GIB, "bytes_scrubbed": 3 * GIB + 512 * MIB,
    "bytes_verified": 3 * GIB + 512 * MIB, "fraction": 3.5 / 288, "dirty_words_before": 1234,
    "n_bad": 0, "first_bad_byte": NONE64, "bits_bad": 0, "t_total_ms": 41.6, "msg": "ok",
}
CTRL_LDS_OK = {
    "ok": True, "rc": 0, "cus_expected": 256, "cus_seen": 255, "xcds_seen": 8, "rounds": 4,
    "lds_bytes": LDS, "workgroups": 1024, "bytes_scrubbed": 1024 * LDS,
    "dirty_words_before": 4321, "dirty_workgroups": 9, "n_bad": 0, "guard_bad": 0,
    "recheck_dirty_words": 0, "first_bad_word": (1 << 32) - 1, "bits_bad": 0, "xcd": -1,
    "se": -1, "sh": -1, "cu": -1, "gpu_ms": 0.05, "t_total_ms": 1.2, "msg": "ok",
}
CTRL_LDS_RESIDUE = dict(CTRL_LDS_OK, ok=False, rc=-42, n_bad=2, first_bad_word=1024,
                        bits_bad=0x00010001, xcd=3, se=1, sh=0, cu=5,
                        msg="LDS residue at xcd=3 se=1 sh=0 cu=5: first_bad_word 1024")
CTRL_LDS_COVERAGE = dict(CTRL_LDS_OK, ok=False, rc=-43, cus_seen=200,
                         msg="LDS scrub reached 200 of 256 CUs after 4 rounds")


def _merged(lds):
    return scrub_mod.merge_lds_result(OK_RESULT, lds)


class _Scrub:
    """A fake ops.scrub that answers from a list (the last answer repeats)."""

    def __init__(self, world, answers):
        self.world, self.answers, self.calls = world, list(answers), 0
        world.ops.scrub = self

    def __call__(self, node, device_id):
        self.calls += 1
        self.world.ops.calls.append(("scrub", node, device_id))
        answer = self.answers[min(self.calls, len(self.answers)) - 1]
        return dict(answer) if answer is not None else None


def _online(world, name="gpu-1", **kw):
    make_node(world.client, "node0")
    world.client.create(make_resource(name, **kw))
    world.resource_rec.reconcile(name)
    world.resource_rec.reconcile(name)
    assert world.client.get(ComposableResource, name).status.state == "Online"


def _start_detach(world, name="gpu-1"):
    world.client.delete(ComposableResource, name)
    world.resource_rec.reconcile(name)  # Online → Detaching
    assert world.client.get(ComposableResource, name).status.state == "Detaching"


def _reasons(world):
    return [e.reason for e in sorted(world.client.list(Event), key=lambda e: e.first_seen)]


def _events(world, reason):
    return [e for e in world.client.list(Event) if e.reason == reason]


def _counter(metrics, reason):
    return metrics.scrub_failures_total.labels(reason=reason)._value.get()


def test_scrubbed_event_gains_the_lds_clause(mock_world):
    _online(mock_world)
    _Scrub(mock_world, [_merged(CTRL_LDS_OK)])
    metrics = mock_world.resource_rec.metrics
    bytes_before = metrics.scrub_bytes_total._value.get()
    _start_detach(mock_world)
    device_id = mock_world.client.get(ComposableResource, "gpu-1").status.device_id
    mock_world.resource_rec.reconcile("gpu-1")
    (event,) = _events(mock_world, "Scrubbed")
    assert event.type == "Normal"
    assert event.message == (
        f"scrubbed 3.50 GiB (1.2 % of VRAM) of device {device_id}, verified; "
        "1234 dirty words found before; 42 ms"
        "; LDS of 255 of 256 CUs cleared (163840 KiB), 4321 dirty LDS words found before"
    )
    # the byte counter is VRAM's, as its help text says
    assert metrics.scrub_bytes_total._value.get() - bytes_before == 3 * GIB + 512 * MIB
    assert _reasons(mock_world) == ["AttachStarted", "FabricAttached", "Online", "DetachStarted",
                                    "Scrubbed", "Detached"]


def test_scrubbed_event_without_the_lds_key_is_unchanged(mock_world):
    _online(mock_world)
    _Scrub(mock_world, [OK_RESULT])
    _start_detach(mock_world)
    device_id = mock_world.client.get(ComposableResource, "gpu-1").status.device_id
    mock_world.resource_rec.reconcile("gpu-1")
    (event,) = _events(mock_world, "Scrubbed")
    assert event.message == (
        f"scrubbed 3.50 GiB (1.2 % of VRAM) of device {device_id}, verified; "
        "1234 dirty words found before; 42 ms"
    )


@pytest.mark.parametrize("lds,reason,lead", [
    (CTRL_LDS_RESIDUE, "lds_residue",
     "xcd=3 se=1 sh=0 cu=5 first_bad_word=1024 bits_bad=0x00010001 n_bad=2 "),
    (CTRL_LDS_COVERAGE, "lds_coverage",
     "xcd=-1 se=-1 sh=-1 cu=-1 first_bad_word=4294967295 bits_bad=0x00000000 n_bad=0 "),
])
def test_lds_failure_reasons(mock_world, lds, reason, lead):
    _online(mock_world)
    scrub = _Scrub(mock_world, [_merged(lds), _merged(CTRL_LDS_OK)])
    metrics = mock_world.resource_rec.metrics
    before = {r: _counter(metrics, r) for r in ("lds_residue", "lds_coverage", "residue", "error")}
    _start_detach(mock_world)
    mock_world.ops.calls.clear()
    with pytest.raises(ScrubFailed, match=f"failed: {reason} "):
        mock_world.resource_rec.reconcile("gpu-1")
    after = {r: _counter(metrics, r) for r in before}
    assert {r: after[r] - before[r] for r in before} == {
        r: (1 if r == reason else 0) for r in before}
    assert "drain" not in [c[0] for c in mock_world.ops.calls]
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Detaching"
    assert got.status.error.startswith(
        f"scrub of device {got.status.device_id} failed: {reason} " + lead)
    assert got.status.error.endswith(": " + lds["msg"])
    (event,) = _events(mock_world, "ScrubFailed")
    assert event.type == "Warning" and event.message == got.status.error
    assert _events(mock_world, "Scrubbed") == []
    # the next reconcile scrubs again, passes, and the detach goes on
    mock_world.resource_rec.reconcile("gpu-1")
    assert scrub.calls == 2 and "drain" in [c[0] for c in mock_world.ops.calls]
    assert len(_events(mock_world, "Scrubbed")) == 1


def test_lds_reasons_from_a_result_without_the_nested_object(mock_world):
    """rc alone names the reason (an agent's error shape has no "lds")."""
    _online(mock_world)
    _Scrub(mock_world, [dict(ok=False, rc=-42, msg="LDS residue")])
    before = _counter(mock_world.resource_rec.metrics, "lds_residue")
    _start_detach(mock_world)
    with pytest.raises(ScrubFailed, match="failed: lds_residue xcd=None .*: LDS residue$"):
        mock_world.resource_rec.reconcile("gpu-1")
    assert _counter(mock_world.resource_rec.metrics, "lds_residue") - before == 1


def test_vram_failure_with_an_lds_object_keeps_its_reason_and_message(mock_world):
    _online(mock_world)
    vram_bad = dict(OK_RESULT, ok=False, rc=-40, n_bad=3, first_bad_byte=4096,
                    bits_bad=0x00010001, msg="residue after scrub: 3 bad words")
    _Scrub(mock_world, [scrub_mod.merge_lds_result(vram_bad, CTRL_LDS_OK)])
    _start_detach(mock_world)
    with pytest.raises(ScrubFailed) as exc:
        mock_world.resource_rec.reconcile("gpu-1")
    assert " failed: residue first_bad_byte=4096 bits_bad=0x00010001 n_bad=3 " in str(exc.value)


def test_failed_lds_scrub_with_force_detach_warns_and_detaches(mock_world):
    _online(mock_world, force_detach=True)
    scrub = _Scrub(mock_world, [_merged(CTRL_LDS_RESIDUE)])
    metrics = mock_world.resource_rec.metrics
    before = _counter(metrics, "lds_residue")
    _start_detach(mock_world)
    for _ in range(3):
        mock_world.resource_rec.reconcile("gpu-1")
    assert mock_world.client.try_get(ComposableResource, "gpu-1") is None
    assert scrub.calls == 1
    (event,) = _events(mock_world, "ScrubFailed")
    assert event.type == "Warning" and "lds_residue xcd=3 se=1 sh=0 cu=5" in event.message
    assert event.message.endswith("force_detach: detaching anyway")
    assert _counter(metrics, "lds_residue") - before == 1
    reasons = _reasons(mock_world)
    assert "Detached" in reasons and "Scrubbed" not in reasons and "ReconcileError" not in reasons


# -- croagent scrub --lds without a GPU ------------------------------------------------


@pytest.fixture(scope="module")
def agent():
    from cro_amd.hip import build as hip_build

    if not os.path.exists(AGENT):
        hip_build.build()
    if not os.path.exists(hip_build.SCRUB_OUT):
        hip_build.build_scrub()
    if not os.path.exists(hip_build.LDS_SCRUB_OUT):
        hip_build.build_lds_scrub()
    return AGENT


def test_croagent_scrub_lds_without_a_gpu_reports_json_and_fails(agent):
    if os.path.exists("/dev/kfd"):
        pytest.skip("this host has a GPU; the agent's scrub on it is tests/test_lds_scrub_gpu.py")
    for argv in (["scrub", "--lds"], ["scrub", "--device", "0", "--max-mib", "64", "--lds"],
                 ["scrub", "--bdf", "0000:5a:00.0", "--lds", "--lds-min-cu-fraction", "0.5"]):
        proc = subprocess.run([agent, *argv], capture_output=True, text=True, timeout=60)
        assert proc.returncode == 1, (argv, proc.stdout, proc.stderr)
        lines = proc.stdout.strip().splitlines()
        assert len(lines) == 1, proc.stdout
        data = json.loads(lines[0])
        assert data["ok"] is False and data["rc"] == -1 and data["msg"], data


def test_croagent_without_the_lds_library_says_so_and_serves_the_rest(agent, tmp_path,
                                                                      monkeypatch):
    """An agent built by the build's own recipe beside libcroprobe.so only,
    then beside libcroscrub.so too: ``scrub --lds`` names the library that is
    missing and scrubs nothing; every other subcommand works."""
    from cro_amd.hip import build as hip_build

    (tmp_path / "agent").mkdir()
    (tmp_path / "hip").mkdir()
    lone = tmp_path / "agent" / "croagent"
    shutil.copy(hip_build.OUT, tmp_path / "hip" / "libcroprobe.so")
    monkeypatch.setattr(hip_build, "HIP_DIR", str(tmp_path / "hip"))
    monkeypatch.setattr(hip_build, "AGENT_OUT", str(lone))
    hip_build.build_agent(force=True)

    def scrub_lds():
        proc = subprocess.run([str(lone), "scrub", "--lds"], capture_output=True, text=True,
                              timeout=60)
        assert proc.returncode == 1
        (line,) = proc.stdout.strip().splitlines()
        data = json.loads(line)
        assert set(data) == {"ok", "rc", "msg"} and data["ok"] is False and data["rc"] == -1
        return data["msg"]

    assert scrub_lds().startswith("libcroscrub.so not available: ")
    shutil.copy(hip_build.SCRUB_OUT, tmp_path / "hip" / "libcroscrub.so")
    assert scrub_lds().startswith("libcroldsscrub.so not available: ")
    proc = subprocess.run([str(lone), "list", "--sysroot", str(tmp_path)], capture_output=True,
                          text=True, timeout=60)
    assert proc.returncode == 0 and json.loads(proc.stdout) == {"gpus": []}
    proc = subprocess.run([str(lone), "pids", "--sysroot", str(tmp_path)], capture_output=True,
                          text=True, timeout=60)
    assert proc.returncode == 0 and json.loads(proc.stdout) == {"pids": []}


# -- build ---------------------------------------------------------------------------


def test_build_lds_scrub_inputs_and_command_line(tmp_path, monkeypatch):
    from cro_amd.hip import build as hip_build

    inputs = [hip_build.LDS_SCRUB_SRC] + hip_build.LDS_SCRUB_HEADERS
    assert {os.path.basename(p) for p in inputs} == {
        "ldsscrub.hip", "croldsscrub.h", "crohost.h", "crocoverage.h"}
    assert all(os.path.exists(p) for p in inputs)
    assert os.path.basename(hip_build.LDS_SCRUB_OUT) == "libcroldsscrub.so"
    # every quoted include of the source, and of the headers it includes, is an input
    for path in inputs:
        with open(path) as f:
            for name in re.findall(r'#include "([^"]+)"', f.read()):
                assert os.path.join(HIP_DIR, name) in inputs, (path, name)
    # the three older input lists do not know the new files
    new = set(inputs[:2])
    assert not new & set(hip_build.ALL_SRCS + hip_build.ALL_HEADERS)
    assert not new & set([hip_build.SCRUB_SRC] + hip_build.SCRUB_HEADERS)
    assert not new & {hip_build.AGENT_SRC, hip_build.HEADERS[0], hip_build.COVERAGE_HEADER,
                      hip_build.OUT}

    files = {}
    for path in inputs + [hip_build.SRC, hip_build.SCRUB_SRC, hip_build.AGENT_SRC]:
        name = os.path.basename(path)
        files[name] = tmp_path / name
        files[name].write_text("")
        os.utime(files[name], (100, 100))
    out = tmp_path / "libcroldsscrub.so"
    monkeypatch.setattr(hip_build, "LDS_SCRUB_SRC", str(files["ldsscrub.hip"]))
    monkeypatch.setattr(hip_build, "LDS_SCRUB_HEADERS",
                        [str(files[os.path.basename(p)]) for p in hip_build.LDS_SCRUB_HEADERS])
    monkeypatch.setattr(hip_build, "LDS_SCRUB_OUT", str(out))
    commands = []

    def fake_run(argv, check):
        commands.append(argv)
        target = argv[argv.index("-o") + 1]
        open(target, "a").close()
        os.utime(target, (400, 400))

    monkeypatch.setattr(hip_build.subprocess, "run", fake_run)
    assert hip_build.build_lds_scrub() == str(out)  # missing: built
    assert commands == [[hip_build.HIPCC, *hip_build.DEVICE_FLAGS, "-fPIC", "-shared",
                         str(files["ldsscrub.hip"]), "-o", str(out)]]
    assert hip_build.DEVICE_FLAGS == ["--offload-arch=gfx950", "-O3"]
    commands.clear()
    hip_build.build_lds_scrub()
    assert commands == []  # up to date
    for name in [os.path.basename(p) for p in inputs]:
        os.utime(out, (200, 200))
        os.utime(files[name], (300, 300))
        hip_build.build_lds_scrub()
        assert len(commands) == 1, name
        commands.clear()
        os.utime(files[name], (100, 100))
    os.utime(out, (200, 200))
    for name in ("probe.hip", "scrub.hip", "croagent.cpp"):  # not its inputs
        os.utime(files[name], (300, 300))
    hip_build.build_lds_scrub()
    assert commands == []
    hip_build.build_lds_scrub(force=True)
    assert len(commands) == 1


def test_the_module_and_the_entry_build_all_three_libraries(monkeypatch, capsys):
    import runpy

    from cro_amd.hip import build as hip_build

    built = []
    monkeypatch.setattr(hip_build, "build", lambda force=False: built.append("probe") or "P")
    monkeypatch.setattr(hip_build, "build_scrub", lambda force=False: built.append("scrub") or "S")
    monkeypatch.setattr(hip_build, "build_lds_scrub",
                        lambda force=False: built.append(("lds", force)) or "L")
    entry = runpy.run_path(os.path.join(REPO, "__graft_entry__.py"))
    entry["build"]()
    assert built == ["probe", "scrub", ("lds", True)]
    assert "built L" in capsys.readouterr().out.splitlines()
