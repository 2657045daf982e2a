"""CPU tests of the quick probe's windows entry (``cro_probe_run_windows``,
cro_amd/hip/probe.hip): ``struct CroProbeWindows`` against its ctypes mirror,
in the style of tests/test_probe_quick.py, and the Python plumbing of
``run_probe_windows``.
"""

import ctypes
import subprocess

import pytest

from cro_amd.nodeops import probe as probe_mod
from tests.test_probe_quick import QUICK_KEYS, _build

FIELDS = ["copy_launches", "bf16_iters", "skip_check_launch", "reserved"]


def _struct_main():
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "croprobe.h"', "int main() {",
             '  printf("sizeof %zu\\n", sizeof(CroProbeWindows));']
    for field in FIELDS:
        lines.append(
            f'  printf("{field} %zu %zu\\n", offsetof(CroProbeWindows, {field}), '
            f"sizeof(((CroProbeWindows*)0)->{field}));"
        )
    lines += ["  return 0;", "}"]
    return "\n".join(lines)


def test_windows_struct_layout_matches_ctypes(tmp_path):
    """Every field of the mirror exists in the header at the same offset and
    size, the totals agree (so the header has no extra one), no holes."""
    mirror = probe_mod.CroProbeWindows
    assert [name for name, _ in mirror._fields_] == FIELDS
    exe = _build(tmp_path, "windows_main", _struct_main())
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        parts = line.split()
        if parts[0] == "sizeof":
            assert ctypes.sizeof(mirror) == int(parts[1]), line
        else:
            desc = getattr(mirror, parts[0])
            assert (desc.offset, desc.size) == (int(parts[1]), int(parts[2])), line
        seen += 1
    assert seen == 1 + len(FIELDS)
    end = 0
    for field in FIELDS:
        desc = getattr(mirror, field)
        assert desc.offset == end, field
        end = desc.offset + desc.size
    assert end == ctypes.sizeof(mirror) == 16
    assert bytes(mirror()) == bytes(16)  # every default is 0: the library's windows


class FakeLib:
    def __init__(self, rc=0):
        self.calls = []
        self.rc = rc

    def cro_probe_run(self, device, res):
        res._obj.ok = 1
        return 0

    def cro_probe_run_windows(self, device, windows, res):
        w = windows._obj
        self.calls.append((device, {name: getattr(w, name) for name, _ in w._fields_}))
        res._obj.ok = 1
        res._obj.mfma_f32_exact = 1
        res._obj.hbm_gbps = 5000.0
        res._obj.msg = b"ok"
        return self.rc


def test_run_probe_windows_forwards_the_windows(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(probe_mod, "_lib", fake)
    got = probe_mod.run_probe_windows(3)
    assert fake.calls == [(3, dict.fromkeys(FIELDS, 0))]  # all defaults
    assert list(got) == QUICK_KEYS  # the result shape of run_probe
    assert list(got) == list(probe_mod.run_probe(0))
    assert got["ok"] is True and got["rc"] == 0 and got["mfma_f32_exact"] is True
    assert got["hbm_gbps"] == 5000.0 and got["msg"] == "ok"
    probe_mod.run_probe_windows(1, copy_launches=2, bf16_iters=512, skip_check_launch=1)
    assert fake.calls[1] == (1, {"copy_launches": 2, "bf16_iters": 512, "skip_check_launch": 1,
                                 "reserved": 0})
    probe_mod.run_probe_windows(0, copy_launches=-1, bf16_iters=65537)  # the library refuses
    assert fake.calls[2][1]["copy_launches"] == -1 and fake.calls[2][1]["bf16_iters"] == 65537
    with pytest.raises(TypeError):
        probe_mod.run_probe_windows(0, launches=2)
    fake.rc = -2
    assert probe_mod.run_probe_windows(0, skip_check_launch=1)["ok"] is False  # rc gates ok
