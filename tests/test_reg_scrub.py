"""CPU tests of the register scrub stage: the three C structs against their
Python mirrors and the record aggregation against a Python re-implementation
(through small host programs built with the host C++ compiler — no HIP, no
GPU), the register use of the compiled kernel, the library loader, the
operator flags, the merge of the stages' results, the exec path, the
controller's scrub phase with a register result, the agent's ``scrub --regs``
on a machine without a GPU, and the build of the library."""

import argparse
import ctypes
import json
import logging
import os
import re
import shutil
import subprocess

import pytest

from cro_amd.api.v1alpha1.types import ComposableResource, Event
from cro_amd.hip import build as hip_build
from cro_amd.nodeops import ldsscrub as lds_mod
from cro_amd.nodeops import regscrub as reg_mod
from cro_amd.nodeops import scrub as scrub_mod
from cro_amd.nodeops.amdgpu import ScrubFailed
from tests.conftest import make_node, make_resource

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(REPO, "cro_amd", "hip")
AGENT = os.path.join(REPO, "cro_amd", "agent", "croagent")
MIB = 1 << 20
GIB = 1 << 30
NONE32 = (1 << 32) - 1
NONE64 = (1 << 64) - 1


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

MIRRORS = {"CroRegScrubOpts": reg_mod.CroRegScrubOpts,
           "CroRegScrubResult": reg_mod.CroRegScrubResult,
           "CroRegScrubRecord": reg_mod.CroRegScrubRecord}


def _layout_source():
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "croregscrub.h"',
             "int main() {"]
    for cname, mirror in MIRRORS.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for field, _ in mirror._fields_:
            lines.append(
                f'  printf("{cname} {field} %zu %zu\\n", offsetof({cname}, {field}), '
                f"sizeof((({cname}*)0)->{field}));"
            )
    lines += ['  printf("consts %d %d %d %d\\n", (int)CRO_REG_SCRUB_FIRST_VGPR, '
              "(int)CRO_REG_SCRUB_REGS_PER_LANE, (int)CRO_REG_SCRUB_WAVE_WORDS, "
              "(int)CRO_REG_SCRUB_WAVES);",
              "  return 0;", "}"]
    return "\n".join(lines)


def test_struct_mirrors_match_the_header(tmp_path):
    exe = _build(tmp_path, "reg_layout", _layout_source())
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    seen = set()
    for line in out.splitlines():
        parts = line.split()
        if parts[0] == "consts":
            first, regs, words, waves = (int(v) for v in parts[1:])
            assert (first, regs, words, waves) == (
                reg_mod.FIRST_VGPR, reg_mod.REGS_PER_LANE, reg_mod.WAVE_WORDS, reg_mod.WAVES)
            assert first <= 32 and regs == (256 - first) + 256 and words == regs * 64
            assert waves == 4
            continue
        mirror = MIRRORS[parts[0]]
        if parts[1] == "sizeof":
            assert ctypes.sizeof(mirror) == int(parts[2]), line
        else:
            desc = getattr(mirror, parts[1])
            assert (desc.offset, desc.size) == (int(parts[2]), int(parts[3])), line
        seen.add((parts[0], parts[1]))
    assert len(seen) == sum(len(m._fields_) + 1 for m in MIRRORS.values())
    assert ctypes.sizeof(reg_mod.CroRegScrubRecord) == 32  # eight 32-bit words


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
    names = [f for f, _ in reg_mod.CroRegScrubResult._fields_]
    for want in ("ok", "rc", "simds_expected", "simds_seen", "cus_seen", "xcds_seen", "rounds",
                 "grid", "first_vgpr", "regs_per_lane", "waves", "bytes_scrubbed",
                 "dirty_words_before", "n_bad", "recheck_dirty_words", "first_dirty_word",
                 "first_bad_word", "bits_bad", "xcd", "se", "sh", "cu", "simd", "wave", "gpu_ms",
                 "t_total_ms", "msg"):
        assert want in names, want
    assert names[:2] == ["ok", "rc"]
    assert reg_mod.CroRegScrubResult.msg.size == 256


# -- croregscrub.h aggregation against a Python re-implementation ----------------------

# reads records as lines of eight numbers, prints the aggregate as one line
AGG_SHIM = r"""
#include <cstdio>
#include <vector>
#include "croregscrub.h"

int main() {
  std::vector<CroRegScrubRecord> v;
  CroRegScrubRecord r;
  while (scanf("%u %u %u %u %u %u %u %u", &r.xcc_id, &r.hw_id, &r.dirty_lanes, &r.first_dirty,
               &r.n_bad, &r.first_bad, &r.bits_bad, &r.valid) == 8)
    v.push_back(r);
  const CroRegScrubRecord clean = CRO_REG_SCRUB_CLEAN_RECORD;
  if (clean.valid || clean.dirty_lanes || clean.n_bad || clean.bits_bad ||
      clean.first_dirty != ~0u || clean.first_bad != ~0u)
    return 2;
  CroRegScrubAgg a;
  cro_reg_scrub_aggregate(v.empty() ? nullptr : v.data(), v.size(), &a);
  printf("%llu %llu %llu %llu %llu %lld %d %d %d %d %d %d %d %d %d %u %u %u\n", a.waves,
         a.dirty_words, a.dirty_waves, a.n_bad, a.bad_waves, a.first_bad_index, a.simds_seen,
         a.cus_seen, a.xcds_seen, a.xcd, a.se, a.sh, a.cu, a.simd, a.wave, a.first_dirty_word,
         a.first_bad_word, a.bits_bad);
  return 0;
}
"""
AGG_KEYS = ("waves", "dirty_words", "dirty_waves", "n_bad", "bad_waves", "first_bad_index",
            "simds_seen", "cus_seen", "xcds_seen", "xcd", "se", "sh", "cu", "simd", "wave",
            "first_dirty_word", "first_bad_word", "bits_bad")
REC_KEYS = ("xcc_id", "hw_id", "dirty_lanes", "first_dirty", "n_bad", "first_bad", "bits_bad",
            "valid")
CLEAN = dict(xcc_id=0, hw_id=0, dirty_lanes=0, first_dirty=NONE32, n_bad=0, first_bad=NONE32,
             bits_bad=0, valid=0)


def _rec(xcd, se, sh, cu, simd, slot=0, **kw):
    # bits above 3:0 of XCC_ID are not the XCD; 0x40 is PIPE_ID
    return dict(CLEAN, xcc_id=xcd | 0xABC0,
                hw_id=(se << 13) | (sh << 12) | (cu << 8) | (simd << 4) | slot | 0x40, valid=1,
                **kw)


def py_aggregate(records):
    """croregscrub.h's cro_reg_scrub_aggregate, from its description."""
    a = dict.fromkeys(AGG_KEYS, 0)
    a.update(first_bad_index=-1, xcd=-1, se=-1, sh=-1, cu=-1, simd=-1, wave=-1,
             first_dirty_word=NONE32, first_bad_word=NONE32)
    simds, cus, xcds = set(), set(), set()
    for i, r in enumerate(records):
        if not r["valid"]:
            continue
        a["waves"] += 1
        xcd, hw = r["xcc_id"] & 0xF, r["hw_id"]
        loc = dict(xcd=xcd, se=(hw >> 13) & 7, sh=(hw >> 12) & 1, cu=(hw >> 8) & 0xF,
                   simd=(hw >> 4) & 3)
        cu_key = (loc["xcd"], loc["se"], loc["sh"], loc["cu"])
        cus.add(cu_key)
        simds.add(cu_key + (loc["simd"],))
        xcds.add(xcd)
        if r["dirty_lanes"]:
            a["dirty_words"] += r["dirty_lanes"]
            a["dirty_waves"] += 1
            a["first_dirty_word"] = min(a["first_dirty_word"], r["first_dirty"])
        if not r["n_bad"]:
            continue
        a["bad_waves"] += 1
        a["n_bad"] += r["n_bad"]
        a["bits_bad"] |= r["bits_bad"]
        if a["first_bad_index"] < 0:
            a.update(loc, first_bad_index=i, wave=i % 4, first_bad_word=r["first_bad"])
    a.update(simds_seen=len(simds), cus_seen=len(cus), xcds_seen=len(xcds))
    return a


@pytest.fixture(scope="module")
def agg_shim(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("regagg"), "regagg_shim", AGG_SHIM)

    def run(records):
        text = "".join(" ".join(str(r[k]) for k in REC_KEYS) + "\n" for r in records)
        proc = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr
        return dict(zip(AGG_KEYS, (int(v) for v in proc.stdout.split())))

    return run


def _agg_cases():
    one_cu = [_rec(2, 1, 0, 5, simd, slot=simd) for simd in range(4)]
    mixed = [
        _rec(0, 0, 0, 0, 0, dirty_lanes=31744, first_dirty=0),            # 0
        _rec(0, 0, 0, 0, 3, slot=7, dirty_lanes=3, first_dirty=17),       # 1: same CU, SIMD 3
        dict(CLEAN, n_bad=9, first_bad=1, dirty_lanes=5, bits_bad=0xFF),  # 2: invalid, skipped
        _rec(7, 3, 1, 15, 1, slot=2, n_bad=2, first_bad=1024, bits_bad=0x80000000),  # 3: bad
        _rec(7, 3, 1, 14, 0, n_bad=5, first_bad=3, bits_bad=0x00000001),  # 4: bad, later index
        _rec(1, 0, 0, 0, 0, dirty_lanes=1, first_dirty=31743),            # 5: another XCD
        _rec(0, 0, 1, 0, 0),                                              # 6: another SH
        _rec(0, 0, 0, 0, 0),                                              # 7: record 0's SIMD again
    ]
    whole = [_rec(xcd, se, 0, cu, simd) for _ in range(2) for xcd in range(8) for se in range(4)
             for cu in range(8) for simd in range(4)]
    return {
        "none": [],
        "invalid_only": [dict(CLEAN), dict(CLEAN, n_bad=9, first_bad=1, dirty_lanes=5)],
        "one_cu": one_cu,
        "mixed": mixed,
        "prefix": mixed[:3],
        "tail": mixed[1:6],
        "whole_device_twice": whole,
        "largest_fields": [_rec(15, 7, 1, 15, 3, slot=15, n_bad=1, first_bad=31743)],
    }


@pytest.mark.parametrize("case", sorted(_agg_cases()))
def test_aggregation_matches_the_python_reimplementation(agg_shim, case):
    records = _agg_cases()[case]
    assert agg_shim(records) == py_aggregate(records)


def test_aggregation_hand_made_answers(agg_shim):
    """The answers themselves, so the two implementations cannot be wrong together."""
    cases = _agg_cases()
    a = agg_shim(cases["invalid_only"])
    assert (a["waves"], a["n_bad"], a["dirty_words"], a["first_bad_index"], a["cus_seen"]) == (
        0, 0, 0, -1, 0)
    # four SIMDs of one CU: once per CU, four times per SIMD
    a = agg_shim(cases["one_cu"])
    assert (a["waves"], a["cus_seen"], a["simds_seen"], a["xcds_seen"]) == (4, 1, 4, 1)
    a = agg_shim(cases["mixed"])
    assert (a["waves"], a["cus_seen"], a["simds_seen"], a["xcds_seen"]) == (7, 5, 6, 3)
    assert (a["dirty_words"], a["dirty_waves"], a["first_dirty_word"]) == (31748, 3, 0)
    # the first bad record leads; bits_bad is the OR
    assert (a["n_bad"], a["bad_waves"], a["bits_bad"]) == (7, 2, 0x80000001)
    assert (a["first_bad_index"], a["first_bad_word"], a["wave"]) == (3, 1024, 3)
    assert (a["xcd"], a["se"], a["sh"], a["cu"], a["simd"]) == (7, 3, 1, 15, 1)
    # the lowest dirty offset is a minimum, not the first
    a = agg_shim(cases["tail"])
    assert (a["first_dirty_word"], a["dirty_words"], a["first_bad_index"], a["wave"]) == (
        17, 4, 2, 2)
    a = agg_shim(cases["whole_device_twice"])
    assert (a["waves"], a["cus_seen"], a["simds_seen"], a["xcds_seen"]) == (2048, 256, 1024, 8)


def test_aggregation_shim_under_host_sanitizers(tmp_path):
    """The stand-alone host program, built with ASan and UBSan."""
    try:
        exe = _build(tmp_path, "regagg_san", AGG_SHIM,
                     extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    except subprocess.CalledProcessError as exc:
        pytest.skip(f"host compiler cannot build with sanitizers: {exc.stderr[-200:]}")
    records = _agg_cases()["mixed"]
    text = "".join(" ".join(str(r[k]) for k in REC_KEYS) + "\n" for r in records)
    proc = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert dict(zip(AGG_KEYS, (int(v) for v in proc.stdout.split()))) == py_aggregate(records)
    assert "runtime error" not in proc.stderr and "Sanitizer" not in proc.stderr


# -- the compiled kernel's register use --------------------------------------------------


@pytest.fixture(scope="module")
def reg_asm(tmp_path_factory):
    """regscrub.hip as device assembly, with the flags the library is built with."""
    out = tmp_path_factory.mktemp("asm") / "regscrub.s"
    subprocess.run(
        [hip_build.HIPCC, *hip_build.DEVICE_FLAGS, "-S", "--cuda-device-only",
         hip_build.REG_SCRUB_SRC, "-o", str(out)],
        check=True, capture_output=True, text=True,
    )
    return out.read_text()


def _split_blocks(asm):
    """(lines outside, list of blocks) by the compiler's inline-assembly markers."""
    outside, blocks, current = [], [], None
    for line in asm.splitlines():
        if ";;#ASMSTART" in line:
            assert current is None
            current = []
        elif ";;#ASMEND" in line:
            blocks.append(current)
            current = None
        elif current is not None:
            current.append(line)
        else:
            outside.append(line)
    assert current is None
    return outside, blocks


def _registers(text):
    """Every VGPR and AGPR number an instruction line names, ranges expanded."""
    text = text.split(";")[0]
    found = {"v": set(), "a": set()}
    for kind, lo, hi in re.findall(r"\b([va])\[(\d+):(\d+)\]", text):
        found[kind].update(range(int(lo), int(hi) + 1))
    for kind, n in re.findall(r"\b([va])(\d+)\b", text):
        found[kind].add(int(n))
    return found


def test_kernel_allocates_the_whole_register_file(reg_asm):
    assert re.search(r"^\s*\.amdhsa_next_free_vgpr 512\s*$", reg_asm, re.M)
    assert re.search(r"^\s*\.amdhsa_accum_offset 256\s*$", reg_asm, re.M)
    # nothing of the kernel's lives in memory, where the march would not see it
    assert re.search(r"^\s*\.amdhsa_private_segment_fixed_size 0\s*$", reg_asm, re.M)
    assert re.search(r"^\s*\.vgpr_spill_count:\s+0\s*$", reg_asm, re.M)
    assert re.search(r"^\s*\.amdhsa_group_segment_fixed_size 0\s*$", reg_asm, re.M)


def test_compiler_code_stays_below_the_first_covered_register(reg_asm):
    """The census sees the registers as found, and the self-test's plant
    survives to the census, only if no instruction outside the inline-assembly
    blocks touches a covered register."""
    outside, blocks = _split_blocks(reg_asm)
    assert len(blocks) == 4  # two s_getreg, the march, the low-register overwrite
    for line in outside:
        stripped = line.strip()
        if not stripped or stripped.startswith((".", ";")) or stripped.endswith(":"):
            continue
        regs = _registers(stripped)
        assert not regs["a"], line
        assert all(n < reg_mod.FIRST_VGPR for n in regs["v"]), line


def test_march_names_every_covered_register(reg_asm):
    _, blocks = _split_blocks(reg_asm)
    march = max(blocks, key=len)
    named = {"v": set(), "a": set()}
    written = {"v": set(), "a": set()}
    for line in march:
        regs = _registers(line)
        for kind in "va":
            named[kind] |= regs[kind]
        m = re.match(r"\s*(v_mov_b32|v_accvgpr_write_b32)\s+([va])(\d+),", line)
        if m:
            written[m.group(2)].add(int(m.group(3)))
    covered_v = set(range(reg_mod.FIRST_VGPR, 256))
    assert covered_v <= named["v"] and named["a"] == set(range(256))
    # and the fill writes each of them (the operands the compiler chose lie below)
    assert covered_v <= written["v"] and written["a"] == set(range(256))
    # the last block overwrites exactly the kernel's own registers
    low = {"v": set(), "a": set()}
    for line in blocks[-1]:
        for kind in "va":
            low[kind] |= _registers(line)[kind]
    assert low == {"v": set(range(reg_mod.FIRST_VGPR)), "a": set()}


# -- library loading -----------------------------------------------------------------


def test_load_reg_scrub_library_is_loud_only_where_required(monkeypatch, tmp_path):
    monkeypatch.setattr(reg_mod, "_lib", None)
    monkeypatch.setattr(reg_mod, "_LIB_PATH", str(tmp_path / "libcroregscrub.so"))
    assert reg_mod.load_reg_scrub_library(required=False) is None
    with pytest.raises(RuntimeError, match="libcroregscrub.so missing"):
        reg_mod.load_reg_scrub_library(required=True)
    monkeypatch.setattr(reg_mod, "_gpu_present", lambda: True)
    with pytest.raises(RuntimeError, match="on a GPU node"):
        reg_mod.load_reg_scrub_library()
    monkeypatch.setattr(reg_mod, "_gpu_present", lambda: False)
    assert reg_mod.load_reg_scrub_library() is None
    # run_reg_scrub always requires it
    with pytest.raises(RuntimeError, match="libcroregscrub.so missing"):
        reg_mod.run_reg_scrub(0)
    with pytest.raises(RuntimeError, match="libcroregscrub.so missing"):
        reg_mod.run_reg_scrub_records(0)


def test_opts_take_the_keywords_of_the_struct():
    o = reg_mod._reg_scrub_opts(grid=2, max_rounds=1, skip_recheck=1, fill_word=-1,
                                min_simd_fraction=0.5, selftest_mode=4,
                                selftest_pattern=0x1_0000_0001, selftest_wave=3, selftest_word=77,
                                selftest_bit=31)
    assert (o.grid, o.max_rounds, o.skip_recheck, o.fill_word) == (2, 1, 1, 0xFFFFFFFF)
    assert (o.min_simd_fraction, o.selftest_mode, o.selftest_pattern, o.selftest_wave,
            o.selftest_word, o.selftest_bit, o.reserved) == (0.5, 4, 1, 3, 77, 31, 0)
    with pytest.raises(TypeError):
        reg_mod._reg_scrub_opts(no_such_option=1)


# -- entry point ---------------------------------------------------------------------

SCRUB_ENV = ("CRO_SCRUB_ON_DETACH", "CRO_SCRUB_MAX_MIB", "CRO_SCRUB_RESERVE_MIB",
             "CRO_SCRUB_MIN_FRACTION", "CRO_SCRUB_LDS", "CRO_SCRUB_LDS_MIN_CU_FRACTION",
             "CRO_SCRUB_REGS", "CRO_SCRUB_REGS_MIN_SIMD_FRACTION")


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


def test_regs_flags_default_off(monkeypatch):
    args = _parse([], monkeypatch)
    assert (args.scrub_regs, args.scrub_regs_min_simd_fraction) == ("off", 0.0)


def test_regs_flags_and_environment(monkeypatch):
    args = _parse(["--scrub-on-detach", "on", "--scrub-regs", "on",
                   "--scrub-regs-min-simd-fraction", "0.75"], monkeypatch)
    assert (args.scrub_regs, args.scrub_regs_min_simd_fraction, args.scrub_lds) == (
        "on", 0.75, "off")
    env = {"CRO_SCRUB_ON_DETACH": "on", "CRO_SCRUB_REGS": "on",
           "CRO_SCRUB_REGS_MIN_SIMD_FRACTION": "0.5"}
    args = _parse([], monkeypatch, env)
    assert (args.scrub_on_detach, args.scrub_regs, args.scrub_regs_min_simd_fraction) == (
        "on", "on", 0.5)
    # the flag wins over the environment
    args = _parse(["--scrub-regs", "off", "--scrub-regs-min-simd-fraction", "1"], monkeypatch, env)
    assert (args.scrub_regs, args.scrub_regs_min_simd_fraction) == ("off", 1.0)
    with pytest.raises(SystemExit):
        _parse(["--scrub-regs", "maybe"], monkeypatch)


def test_select_scrub_fn_keywords(monkeypatch):
    from cro_amd.cmd import main as main_mod

    made = []
    monkeypatch.setattr(scrub_mod, "make_scrub_fn", lambda **kw: made.append(kw) or "hook")
    argv = ["--scrub-on-detach", "on", "--scrub-max-mib", "3", "--scrub-min-fraction", "0.25"]
    base = {"max_bytes": 3 * MIB, "reserve_bytes": 0, "min_fraction": 0.25}
    # registers off: today's keywords exactly, whatever the SIMD floor says
    for extra in ([], ["--scrub-regs", "off"], ["--scrub-regs-min-simd-fraction", "0.9"]):
        made.clear()
        assert main_mod.select_scrub_fn(_parse(argv + extra, monkeypatch)) == "hook"
        assert made == [base]
    made.clear()
    main_mod.select_scrub_fn(_parse(argv + ["--scrub-lds", "on", "--scrub-regs", "off"],
                                    monkeypatch))
    assert made == [dict(base, lds=True, lds_min_cu_fraction=0.0)]
    # registers on, without and with the LDS stage
    made.clear()
    args = _parse(argv + ["--scrub-regs", "on", "--scrub-regs-min-simd-fraction", "0.9"],
                  monkeypatch)
    assert main_mod.select_scrub_fn(args) == "hook"
    assert made == [dict(base, regs=True, regs_min_simd_fraction=0.9)]
    made.clear()
    args = _parse(argv + ["--scrub-lds", "on", "--scrub-regs", "on"], monkeypatch)
    main_mod.select_scrub_fn(args)
    assert made == [dict(base, lds=True, lds_min_cu_fraction=0.0, regs=True,
                         regs_min_simd_fraction=0.0)]
    # the scrub off: no hook at all
    made.clear()
    assert main_mod.select_scrub_fn(_parse(["--scrub-regs", "on"], monkeypatch)) is None
    assert made == []


def test_regs_on_with_the_scrub_off_is_a_start_up_error(monkeypatch, capsys):
    from cro_amd.cmd import main as main_mod

    p = _parser(monkeypatch)
    with pytest.raises(SystemExit) as exc:
        main_mod.check_scrub_arguments(p, p.parse_args(["--scrub-regs", "on"]))
    assert exc.value.code == 2
    assert "--scrub-regs on needs --scrub-on-detach on" in capsys.readouterr().err
    # it needs the scrub, not the LDS stage
    for argv in ([], ["--scrub-on-detach", "on"], ["--scrub-on-detach", "on", "--scrub-regs", "on"],
                 ["--scrub-on-detach", "on", "--scrub-regs", "on", "--scrub-lds", "on"]):
        main_mod.check_scrub_arguments(p, p.parse_args(argv))
    # and the operator's own entry refuses to start
    for name in SCRUB_ENV:
        monkeypatch.delenv(name, raising=False)
    with pytest.raises(SystemExit) as exc:
        main_mod.main(["--scrub-regs", "on"])
    assert exc.value.code == 2
    monkeypatch.setenv("CRO_SCRUB_REGS", "on")
    with pytest.raises(SystemExit) as exc:
        main_mod.main([])
    assert exc.value.code == 2


def test_operator_without_the_library_warns_and_goes_on_without_the_stage(monkeypatch, caplog):
    from cro_amd.cmd import main as main_mod

    log = logging.getLogger("test_reg_scrub")
    monkeypatch.setattr(scrub_mod, "make_scrub_fn", lambda **kw: kw)
    monkeypatch.setattr(lds_mod, "load_lds_scrub_library", lambda required=None: object())
    argv = ["--scrub-on-detach", "on", "--scrub-regs", "on", "--scrub-regs-min-simd-fraction",
            "0.5"]
    base = {"max_bytes": 0, "reserve_bytes": 0, "min_fraction": 0.0}
    # the library is there: the stage stays
    monkeypatch.setattr(reg_mod, "load_reg_scrub_library", lambda required=None: object())
    args = _parse(argv, monkeypatch)
    with caplog.at_level(logging.INFO, logger="test_reg_scrub"):
        assert main_mod.drop_unavailable_scrub_stages(args, log) is False
    assert [(r.levelname, r.getMessage()) for r in caplog.records] == [
        ("INFO", "scrub on detach: register scrub on")]
    assert main_mod.select_scrub_fn(args) == dict(base, regs=True, regs_min_simd_fraction=0.5)
    # it is missing, or loading it raises: a warning, and the hook without the stage
    def broken(required=None):
        raise OSError("libamdhip64.so: cannot open shared object file")

    for loader in (lambda required=None: None, broken):
        caplog.clear()
        monkeypatch.setattr(reg_mod, "load_reg_scrub_library", loader)
        args = _parse(argv + ["--scrub-lds", "on"], monkeypatch)
        with caplog.at_level(logging.INFO, logger="test_reg_scrub"):
            assert main_mod.drop_unavailable_scrub_stages(args, log) is True
        assert [(r.levelname, r.getMessage()) for r in caplog.records] == [
            ("INFO", "scrub on detach: LDS scrub on"),
            ("WARNING", "gfx950 register scrub library unavailable; register scrub disabled")]
        assert args.scrub_regs == "off" and args.scrub_lds == "on"
        assert main_mod.select_scrub_fn(args) == dict(base, lds=True, lds_min_cu_fraction=0.0)
    # the stage off: the library is not even looked for
    monkeypatch.setattr(reg_mod, "load_reg_scrub_library", broken)
    args = _parse(["--scrub-on-detach", "on"], monkeypatch)
    caplog.clear()
    assert main_mod.drop_unavailable_scrub_stages(args, log) is False
    assert caplog.records == [] and main_mod.select_scrub_fn(args) == base


# -- merge of the stages' results ---------------------------------------------------------

VRAM_OK = {"ok": True, "rc": 0, "bytes_scrubbed": 64 * MIB, "n_bad": 0, "bits_bad": 0,
           "t_total_ms": 41.6, "msg": "ok"}
VRAM_BAD = dict(VRAM_OK, ok=False, rc=-40, n_bad=3, msg="residue after scrub: 3 bad words")
LDS_OK = {"ok": True, "rc": 0, "cus_expected": 256, "cus_seen": 256, "n_bad": 0, "msg": "ok"}
LDS_BAD = dict(LDS_OK, ok=False, rc=-42, n_bad=2, msg="LDS residue at xcd=3 se=1 sh=0 cu=5")
REGS_OK = {"ok": True, "rc": 0, "simds_expected": 1024, "simds_seen": 1024,
           "bytes_scrubbed": 1024 * 496 * 256, "dirty_words_before": 77, "n_bad": 0,
           "recheck_dirty_words": 0, "msg": "ok"}
REGS_BAD = dict(REGS_OK, ok=False, rc=-44, n_bad=2, first_bad_word=1024, bits_bad=0x10,
                xcd=3, se=1, sh=0, cu=5, simd=2, wave=1,
                msg="register residue at xcd=3 se=1 sh=0 cu=5 simd=2")
REGS_LOW = dict(REGS_OK, ok=False, rc=-45, simds_seen=800,
                msg="register scrub reached 800 of 1024 SIMDs")


class _Gpu:
    pci_bdf = "0000:5a:00.0"


def _patch_stages(monkeypatch, calls, vram, lds, regs, device=3):
    monkeypatch.setattr(scrub_mod, "hip_device_for_bdf", lambda bdf: device)
    monkeypatch.setattr(scrub_mod, "run_scrub",
                        lambda dev, **kw: calls.append(("vram", dev, kw)) or dict(vram))
    monkeypatch.setattr(lds_mod, "run_lds_scrub",
                        lambda dev, **kw: calls.append(("lds", dev, kw)) or dict(lds))
    monkeypatch.setattr(reg_mod, "run_reg_scrub",
                        lambda dev, **kw: calls.append(("regs", dev, kw)) or dict(regs))


@pytest.mark.parametrize("vram,regs,ok,rc,msg", [
    (VRAM_OK, REGS_OK, True, 0, "ok"),
    (VRAM_BAD, REGS_OK, False, -40, VRAM_BAD["msg"]),
    (VRAM_OK, REGS_BAD, False, -44, REGS_BAD["msg"]),
    (VRAM_OK, REGS_LOW, False, -45, REGS_LOW["msg"]),
    (VRAM_BAD, REGS_BAD, False, -40, VRAM_BAD["msg"]),  # the first failure leads
])
def test_make_scrub_fn_merges_the_regs_result(monkeypatch, vram, regs, ok, rc, msg):
    calls = []
    _patch_stages(monkeypatch, calls, vram, LDS_OK, regs)
    fn = scrub_mod.make_scrub_fn(max_bytes=5, reserve_bytes=6, min_fraction=0.5, regs=True,
                                 regs_min_simd_fraction=0.9)
    got = fn(_Gpu())
    # the VRAM scrub first, then the register scrub, both on the device's ordinal; no LDS
    assert calls == [("vram", 3, {"max_bytes": 5, "reserve_bytes": 6, "min_fraction": 0.5}),
                     ("regs", 3, {"min_simd_fraction": 0.9})]
    assert (got["ok"], got["rc"], got["msg"]) == (ok, rc, msg)
    assert got["regs"] == regs
    assert list(got) == list(vram) + ["regs"]
    assert {k: v for k, v in got.items() if k not in ("ok", "rc", "msg", "regs")} == {
        k: v for k, v in vram.items() if k not in ("ok", "rc", "msg")}


@pytest.mark.parametrize("vram,lds,regs,ok,rc,msg", [
    (VRAM_OK, LDS_OK, REGS_OK, True, 0, "ok"),
    (VRAM_OK, LDS_BAD, REGS_OK, False, -42, LDS_BAD["msg"]),
    (VRAM_OK, LDS_BAD, REGS_BAD, False, -42, LDS_BAD["msg"]),
    (VRAM_OK, LDS_OK, REGS_BAD, False, -44, REGS_BAD["msg"]),
    (VRAM_BAD, LDS_BAD, REGS_BAD, False, -40, VRAM_BAD["msg"]),
])
def test_make_scrub_fn_runs_all_three_stages_in_order(monkeypatch, vram, lds, regs, ok, rc, msg):
    calls = []
    _patch_stages(monkeypatch, calls, vram, lds, regs)
    fn = scrub_mod.make_scrub_fn(lds=True, lds_min_cu_fraction=0.5, regs=True)
    got = fn(_Gpu())
    assert calls == [("vram", 3, {"max_bytes": 0, "reserve_bytes": 0, "min_fraction": 0.0}),
                     ("lds", 3, {"min_cu_fraction": 0.5}),
                     ("regs", 3, {"min_simd_fraction": 0.0})]
    assert (got["ok"], got["rc"], got["msg"]) == (ok, rc, msg)
    assert list(got) == list(vram) + ["lds", "regs"]  # "regs" after "lds"
    assert got["lds"] == lds and got["regs"] == regs


def test_make_scrub_fn_without_regs_is_unchanged(monkeypatch):
    calls = []
    _patch_stages(monkeypatch, calls, VRAM_OK, LDS_OK, REGS_OK, device=None)

    def never(dev, **kw):
        raise AssertionError("the register scrub ran with regs off")

    monkeypatch.setattr(reg_mod, "run_reg_scrub", never)
    for fn in (scrub_mod.make_scrub_fn(),
               scrub_mod.make_scrub_fn(regs=False, regs_min_simd_fraction=0.9)):
        assert fn(_Gpu()) == VRAM_OK
    assert calls == [("vram", 0, {"max_bytes": 0, "reserve_bytes": 0, "min_fraction": 0.0})] * 2
    calls.clear()
    got = scrub_mod.make_scrub_fn(lds=True, lds_min_cu_fraction=0.9)(_Gpu())
    assert [c[0] for c in calls] == ["vram", "lds"]
    assert got == scrub_mod.merge_lds_result(VRAM_OK, LDS_OK) and "regs" not in got


# -- exec path -----------------------------------------------------------------------


class _Exec:
    def __init__(self, rc=0, out="", err=""):
        self.answer, self.calls = (rc, out, err), []

    def run(self, node, argv, timeout=None):
        self.calls.append((node, list(argv), timeout))
        return self.answer


def test_scrub_via_exec_argv_with_and_without_regs():
    merged = dict(VRAM_OK, regs=REGS_OK)
    base = ["croagent", "scrub", "--bdf", "0000:5a:00.0"]
    execer = _Exec(0, json.dumps(merged) + "\n")
    assert scrub_mod.scrub_via_exec(execer, "node7", _Gpu(), regs=True) == merged
    assert execer.calls == [("node7", base + ["--regs"], 300)]
    execer = _Exec(0, json.dumps(merged))
    scrub_mod.scrub_via_exec(execer, "node7", _Gpu(), argv_prefix=["chroot", "/x"], max_mib=64,
                             min_fraction=0.9, lds=True, lds_min_cu_fraction=0.75, regs=True,
                             regs_min_simd_fraction=0.5)
    assert execer.calls[0][1] == ["chroot", "/x"] + base + [
        "--max-mib", "64", "--min-fraction", "0.9", "--lds", "--lds-min-cu-fraction", "0.75",
        "--regs", "--regs-min-simd-fraction", "0.5"]
    # without regs: today's argv, and the floor alone adds nothing
    for kw in ({}, {"regs": False}, {"regs_min_simd_fraction": 0.75}):
        execer = _Exec(0, json.dumps(VRAM_OK))
        assert scrub_mod.scrub_via_exec(execer, "node7", _Gpu(), max_mib=64, **kw) == VRAM_OK
        assert execer.calls == [("node7", base + ["--max-mib", "64"], 300)]


def test_make_exec_scrub_fn_passes_only_the_stages_that_are_on(monkeypatch):
    calls = []
    monkeypatch.setattr(scrub_mod, "scrub_via_exec",
                        lambda execer, node, gpu, **kw: calls.append(kw) or {"ok": True})
    base = {"argv_prefix": None, "max_mib": 8, "reserve_mib": None, "min_fraction": 0}
    scrub_mod.make_exec_scrub_fn("x", "node7", max_mib=8)(_Gpu())
    scrub_mod.make_exec_scrub_fn("x", "node7", max_mib=8, regs=False,
                                 regs_min_simd_fraction=1.0)(_Gpu())
    scrub_mod.make_exec_scrub_fn("x", "node7", max_mib=8, lds=True,
                                 lds_min_cu_fraction=1.0)(_Gpu())
    scrub_mod.make_exec_scrub_fn("x", "node7", max_mib=8, regs=True,
                                 regs_min_simd_fraction=1.0)(_Gpu())
    scrub_mod.make_exec_scrub_fn("x", "node7", max_mib=8, lds=True, regs=True)(_Gpu())
    assert calls == [
        base, base, dict(base, lds=True, lds_min_cu_fraction=1.0),
        dict(base, regs=True, regs_min_simd_fraction=1.0),
        dict(base, lds=True, lds_min_cu_fraction=0.0, regs=True, regs_min_simd_fraction=0.0)]
    # and the argv that comes of it
    monkeypatch.undo()
    execer = _Exec(0, json.dumps(VRAM_OK))
    scrub_mod.make_exec_scrub_fn(execer, "node7", max_mib=8, regs=True,
                                 regs_min_simd_fraction=1.0)(_Gpu())
    scrub_mod.make_exec_scrub_fn(execer, "node7", max_mib=8)(_Gpu())
    argv0 = ["croagent", "scrub", "--bdf", "0000:5a:00.0", "--max-mib", "8"]
    assert [c[1] for c in execer.calls] == [
        argv0 + ["--regs", "--regs-min-simd-fraction", "1.0"], argv0]


def test_scrub_via_exec_passes_regs_error_shapes_through():
    failed = dict(VRAM_OK, ok=False, rc=-44, msg=REGS_BAD["msg"], regs=REGS_BAD)
    assert scrub_mod.scrub_via_exec(_Exec(1, json.dumps(failed)), "n", _Gpu(),
                                    regs=True) == failed
    missing = {"ok": False, "rc": -1, "msg": "libcroregscrub.so not available: no such file"}
    assert scrub_mod.scrub_via_exec(_Exec(1, json.dumps(missing)), "n", _Gpu(),
                                    regs=True) == missing
    assert scrub_mod.scrub_via_exec(_Exec(127, "", "croagent: not found\n"), "n", _Gpu(),
                                    regs=True) == {
        "ok": False, "rc": 127, "msg": "croagent: not found"}


# -- controller ----------------------------------------------------------------------

OK_RESULT = {
    "ok": True, "rc": 0, "vram_total": 288 * GIB, "bytes_scrubbed": 3 * GIB + 512 * MIB,
    "bytes_verified": 3 * GIB + 512 * MIB, "fraction": 3.5 / 288, "dirty_words_before": 1234,
    "n_bad": 0, "first_bad_byte": NONE64, "bits_bad": 0, "t_total_ms": 41.6, "msg": "ok",
}
CTRL_LDS_OK = {
    "ok": True, "rc": 0, "cus_expected": 256, "cus_seen": 255, "bytes_scrubbed": 1024 * 163840,
    "dirty_words_before": 4321, "n_bad": 0, "recheck_dirty_words": 0, "msg": "ok",
}
CTRL_REGS_OK = {
    "ok": True, "rc": 0, "simds_expected": 1024, "simds_seen": 1020, "cus_seen": 255,
    "xcds_seen": 8, "rounds": 4, "grid": 256, "first_vgpr": 16, "regs_per_lane": 496,
    "waves": 4096, "bytes_scrubbed": 4096 * 496 * 256, "dirty_words_before": 987,
    "dirty_waves": 9, "n_bad": 0, "recheck_dirty_words": 0, "first_dirty_word": 5,
    "first_bad_word": NONE32, "bits_bad": 0, "bad_waves": 0, "xcd": -1, "se": -1, "sh": -1,
    "cu": -1, "simd": -1, "wave": -1, "gpu_ms": 0.05, "t_total_ms": 1.2, "msg": "ok",
}
CTRL_REGS_RESIDUE = dict(CTRL_REGS_OK, ok=False, rc=-44, n_bad=2, first_bad_word=1024,
                         bits_bad=0x00010001, bad_waves=1, xcd=3, se=1, sh=0, cu=5, simd=2,
                         wave=1,
                         msg="register residue at xcd=3 se=1 sh=0 cu=5 simd=2: first_bad_word 1024")
CTRL_REGS_COVERAGE = dict(CTRL_REGS_OK, ok=False, rc=-45, simds_seen=800,
                          msg="register scrub reached 800 of 1024 SIMDs after 4 rounds")


def _merged(regs, lds=None):
    merged = OK_RESULT if lds is None else scrub_mod.merge_lds_result(OK_RESULT, lds)
    return scrub_mod.merge_regs_result(merged, regs)


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


REGS_CLAUSE = ("; vector registers of 1020 of 1024 SIMDs cleared (507904 KiB), "
               "987 dirty register words found before")
LDS_CLAUSE = "; LDS of 255 of 256 CUs cleared (163840 KiB), 4321 dirty LDS words found before"


@pytest.mark.parametrize("lds,tail", [(None, REGS_CLAUSE), (CTRL_LDS_OK, LDS_CLAUSE + REGS_CLAUSE)])
def test_scrubbed_event_gains_the_regs_clause(mock_world, lds, tail):
    _online(mock_world)
    _Scrub(mock_world, [_merged(CTRL_REGS_OK, lds)])
    metrics = mock_world.resource_rec.metrics
    bytes_before = metrics.scrub_bytes_total._value.get()
    _start_detach(mock_world)
    device_id = mock_world.client.get(ComposableResource, "gpu-1").status.device_id
    mock_world.resource_rec.reconcile("gpu-1")
    (event,) = _events(mock_world, "Scrubbed")
    assert event.type == "Normal"
    assert event.message == (
        f"scrubbed 3.50 GiB (1.2 % of VRAM) of device {device_id}, verified; "
        "1234 dirty words found before; 42 ms" + tail
    )
    # the byte counter is VRAM's, as its help text says
    assert metrics.scrub_bytes_total._value.get() - bytes_before == 3 * GIB + 512 * MIB
    assert _reasons(mock_world) == ["AttachStarted", "FabricAttached", "Online", "DetachStarted",
                                    "Scrubbed", "Detached"]


@pytest.mark.parametrize("regs,reason,lead", [
    (CTRL_REGS_RESIDUE, "reg_residue",
     "xcd=3 se=1 sh=0 cu=5 simd=2 wave=1 first_bad_word=1024 bits_bad=0x00010001 n_bad=2 "
     "recheck_dirty_words=0 simds_seen=1020/1024: "),
    (CTRL_REGS_COVERAGE, "reg_coverage",
     "xcd=-1 se=-1 sh=-1 cu=-1 simd=-1 wave=-1 first_bad_word=4294967295 bits_bad=0x00000000 "
     "n_bad=0 recheck_dirty_words=0 simds_seen=800/1024: "),
])
def test_regs_failure_reasons_keep_the_device(mock_world, regs, reason, lead):
    _online(mock_world)
    scrub = _Scrub(mock_world, [_merged(regs), _merged(CTRL_REGS_OK)])
    metrics = mock_world.resource_rec.metrics
    labels = ("reg_residue", "reg_coverage", "lds_residue", "lds_coverage", "residue", "error")
    before = {r: _counter(metrics, r) for r in labels}
    _start_detach(mock_world)
    mock_world.ops.calls.clear()
    with pytest.raises(ScrubFailed, match=f"failed: {reason} "):
        mock_world.resource_rec.reconcile("gpu-1")
    after = {r: _counter(metrics, r) for r in before}
    assert {r: after[r] - before[r] for r in before} == {
        r: (1 if r == reason else 0) for r in before}
    # the device stays on the node
    assert "drain" not in [c[0] for c in mock_world.ops.calls]
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Detaching"
    assert got.status.error == (
        f"scrub of device {got.status.device_id} failed: {reason} " + lead + regs["msg"])
    (event,) = _events(mock_world, "ScrubFailed")
    assert event.type == "Warning" and event.message == got.status.error
    assert _events(mock_world, "Scrubbed") == []
    # the next reconcile scrubs again, passes, and the detach goes on
    mock_world.resource_rec.reconcile("gpu-1")
    assert scrub.calls == 2 and "drain" in [c[0] for c in mock_world.ops.calls]
    assert len(_events(mock_world, "Scrubbed")) == 1


def test_regs_reasons_from_a_result_without_the_nested_object(mock_world):
    """rc alone names the reason (an agent's error shape has no "regs")."""
    _online(mock_world)
    _Scrub(mock_world, [dict(ok=False, rc=-44, msg="register residue")])
    before = _counter(mock_world.resource_rec.metrics, "reg_residue")
    _start_detach(mock_world)
    with pytest.raises(ScrubFailed, match="failed: reg_residue xcd=None .*: register residue$"):
        mock_world.resource_rec.reconcile("gpu-1")
    assert _counter(mock_world.resource_rec.metrics, "reg_residue") - before == 1


def test_lds_failure_with_a_regs_object_keeps_its_reason(mock_world):
    _online(mock_world)
    lds_bad = dict(CTRL_LDS_OK, ok=False, rc=-42, n_bad=2, first_bad_word=7, bits_bad=1, xcd=3,
                   se=1, sh=0, cu=5, msg="LDS residue at xcd=3")
    _Scrub(mock_world, [_merged(CTRL_REGS_RESIDUE, lds_bad)])
    _start_detach(mock_world)
    with pytest.raises(ScrubFailed, match="failed: lds_residue xcd=3 se=1 sh=0 cu=5 "):
        mock_world.resource_rec.reconcile("gpu-1")


def test_failed_regs_scrub_with_force_detach_warns_and_detaches(mock_world):
    _online(mock_world, force_detach=True)
    scrub = _Scrub(mock_world, [_merged(CTRL_REGS_RESIDUE)])
    metrics = mock_world.resource_rec.metrics
    before = _counter(metrics, "reg_residue")
    _start_detach(mock_world)
    for _ in range(3):
        mock_world.resource_rec.reconcile("gpu-1")
    assert mock_world.client.try_get(ComposableResource, "gpu-1") is None
    assert scrub.calls == 1
    (event,) = _events(mock_world, "ScrubFailed")
    assert event.type == "Warning"
    assert "reg_residue xcd=3 se=1 sh=0 cu=5 simd=2" in event.message
    assert event.message.endswith("force_detach: detaching anyway")
    assert _counter(metrics, "reg_residue") - before == 1
    reasons = _reasons(mock_world)
    assert "Detached" in reasons and "Scrubbed" not in reasons and "ReconcileError" not in reasons


def test_metric_help_names_the_two_reasons():
    from cro_amd.metrics import Metrics

    doc = Metrics().scrub_failures_total._documentation
    for word in ("reg_residue", "reg_coverage", "lds_residue", "residue", "error"):
        assert word in doc


# -- croagent scrub --regs without a GPU ------------------------------------------------


@pytest.fixture(scope="module")
def agent():
    if not os.path.exists(AGENT):
        hip_build.build()
    if not os.path.exists(hip_build.SCRUB_OUT):
        hip_build.build_scrub()
    if not os.path.exists(hip_build.LDS_SCRUB_OUT):
        hip_build.build_lds_scrub()
    if not os.path.exists(hip_build.REG_SCRUB_OUT):
        hip_build.build_reg_scrub()
    return AGENT


def test_croagent_scrub_regs_without_a_gpu_reports_json_and_fails(agent):
    if os.path.exists("/dev/kfd"):
        pytest.skip("this host has a GPU; the agent's scrub on it is tests/test_reg_scrub_gpu.py")
    for argv in (["scrub", "--regs"], ["scrub", "--device", "0", "--max-mib", "64", "--regs"],
                 ["scrub", "--bdf", "0000:5a:00.0", "--lds", "--regs",
                  "--regs-min-simd-fraction", "0.5"]):
        proc = subprocess.run([agent, *argv], capture_output=True, text=True, timeout=60)
        assert proc.returncode == 1, (argv, proc.stdout, proc.stderr)
        lines = proc.stdout.strip().splitlines()
        assert len(lines) == 1, proc.stdout
        data = json.loads(lines[0])
        assert data["ok"] is False and data["rc"] == -1 and data["msg"], data


def test_croagent_without_the_regs_library_says_so_and_scrubs_nothing(agent, tmp_path,
                                                                      monkeypatch):
    """An agent built by the build's own recipe beside libcroprobe.so and
    libcroscrub.so only: ``scrub --regs`` names the library that is missing
    before anything runs."""
    (tmp_path / "agent").mkdir()
    (tmp_path / "hip").mkdir()
    lone = tmp_path / "agent" / "croagent"
    shutil.copy(hip_build.OUT, tmp_path / "hip" / "libcroprobe.so")
    shutil.copy(hip_build.SCRUB_OUT, tmp_path / "hip" / "libcroscrub.so")
    monkeypatch.setattr(hip_build, "HIP_DIR", str(tmp_path / "hip"))
    monkeypatch.setattr(hip_build, "AGENT_OUT", str(lone))
    hip_build.build_agent(force=True)

    def scrub(*flags):
        proc = subprocess.run([str(lone), "scrub", *flags], capture_output=True, text=True,
                              timeout=60)
        assert proc.returncode == 1
        (line,) = proc.stdout.strip().splitlines()
        data = json.loads(line)
        assert set(data) == {"ok", "rc", "msg"} and data["ok"] is False and data["rc"] == -1
        return data["msg"]

    assert scrub("--regs").startswith("libcroregscrub.so not available: ")
    assert scrub("--lds", "--regs").startswith("libcroldsscrub.so not available: ")
    shutil.copy(hip_build.LDS_SCRUB_OUT, tmp_path / "hip" / "libcroldsscrub.so")
    assert scrub("--lds", "--regs").startswith("libcroregscrub.so not available: ")


# -- build ---------------------------------------------------------------------------


def test_build_reg_scrub_inputs_and_command_line(tmp_path, monkeypatch):
    inputs = [hip_build.REG_SCRUB_SRC] + hip_build.REG_SCRUB_HEADERS
    assert {os.path.basename(p) for p in inputs} == {
        "regscrub.hip", "croregscrub.h", "crohost.h", "crocoverage.h"}
    assert all(os.path.exists(p) for p in inputs)
    assert os.path.basename(hip_build.REG_SCRUB_OUT) == "libcroregscrub.so"
    # every quoted include of the source, and of the headers it includes, is an input
    for path in inputs:
        with open(path) as f:
            for name in re.findall(r'#include "([^"]+)"', f.read()):
                assert os.path.join(HIP_DIR, name) in inputs, (path, name)
    # the older input lists do not know the new files
    new = set(inputs[:2])
    assert not new & set(hip_build.ALL_SRCS + hip_build.ALL_HEADERS)
    assert not new & set([hip_build.SCRUB_SRC] + hip_build.SCRUB_HEADERS)
    assert not new & set([hip_build.LDS_SCRUB_SRC] + hip_build.LDS_SCRUB_HEADERS)

    files = {}
    for path in inputs + [hip_build.SRC, hip_build.SCRUB_SRC, hip_build.LDS_SCRUB_SRC,
                          hip_build.LDS_SCRUB_HEADERS[0], hip_build.AGENT_SRC]:
        name = os.path.basename(path)
        files[name] = tmp_path / name
        files[name].write_text("")
        os.utime(files[name], (100, 100))
    out = tmp_path / "libcroregscrub.so"
    monkeypatch.setattr(hip_build, "REG_SCRUB_SRC", str(files["regscrub.hip"]))
    monkeypatch.setattr(hip_build, "REG_SCRUB_HEADERS",
                        [str(files[os.path.basename(p)]) for p in hip_build.REG_SCRUB_HEADERS])
    monkeypatch.setattr(hip_build, "REG_SCRUB_OUT", str(out))
    commands = []

    def fake_run(argv, check):
        commands.append(argv)
        target = argv[argv.index("-o") + 1]
        open(target, "a").close()
        os.utime(target, (400, 400))

    monkeypatch.setattr(hip_build.subprocess, "run", fake_run)
    assert hip_build.build_reg_scrub() == str(out)  # missing: built
    assert commands == [[hip_build.HIPCC, *hip_build.DEVICE_FLAGS, "-fPIC", "-shared",
                         str(files["regscrub.hip"]), "-o", str(out)]]
    commands.clear()
    hip_build.build_reg_scrub()
    assert commands == []  # up to date
    for name in [os.path.basename(p) for p in inputs]:
        os.utime(out, (200, 200))
        os.utime(files[name], (300, 300))
        hip_build.build_reg_scrub()
        assert len(commands) == 1, name
        commands.clear()
        os.utime(files[name], (100, 100))
    os.utime(out, (200, 200))
    for name in ("probe.hip", "scrub.hip", "ldsscrub.hip", "croldsscrub.h", "croagent.cpp"):
        os.utime(files[name], (300, 300))  # not its inputs
    hip_build.build_reg_scrub()
    assert commands == []
    hip_build.build_reg_scrub(force=True)
    assert len(commands) == 1


def test_the_module_and_the_entry_build_all_four_libraries(monkeypatch, capsys):
    import runpy

    built = []
    monkeypatch.setattr(hip_build, "build", lambda force=False: built.append("probe") or "P")
    monkeypatch.setattr(hip_build, "build_scrub", lambda force=False: built.append("scrub") or "S")
    monkeypatch.setattr(hip_build, "build_lds_scrub",
                        lambda force=False: built.append(("lds", force)) or "L")
    monkeypatch.setattr(hip_build, "build_reg_scrub",
                        lambda force=False: built.append(("regs", force)) or "R")
    entry = runpy.run_path(os.path.join(REPO, "__graft_entry__.py"))
    entry["build"]()
    assert built == ["probe", "scrub", ("lds", True), ("regs", True)]
    assert "built R" in capsys.readouterr().out.splitlines()
    # python -m cro_amd.hip.build: the fourth path it prints
    built.clear()
    monkeypatch.setattr("sys.argv", ["build"])
    runpy.run_path(hip_build.__file__, run_name="not_main")  # importable without building
    assert built == []
    with open(hip_build.__file__) as f:
        main_block = f.read().split('if __name__ == "__main__":')[1]
    assert main_block.strip().splitlines()[-1].strip() == (
        'print(build_reg_scrub(force="--force" in sys.argv))')
