"""GPU-marked tests of the quick probe as one submission with one wait
(cro_amd/hip/probe.hip): constants cached in the context, the in-stream
poison of the result tile, the windows entry and the event-timed sections.

The rate floors are those tests/test_gpu.py asserts of a healthy device
(2000 GB/s, 500 TF).  The exact gate fires through data alone: one flipped
bit of a per-call copy of the expected tile, or a tile the check kernel was
not launched to write.  Nothing on the GPU is provoked.
"""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE_BAD = {"n_bad": 0, "first_bad": 2 ** 64 - 1}


def _require_gpu():
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU (KFD) on this host")


def _child(code, timeout):
    """Run ``code`` in a fresh interpreter with a time limit of its own; the
    last line it prints is JSON."""
    proc = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True,
                          text=True, timeout=timeout)
    assert proc.returncode == 0, (proc.returncode, proc.stdout[-2000:], proc.stderr[-2000:])
    return json.loads(proc.stdout.strip().splitlines()[-1])


def _healthy(res):
    return (res["rc"] == 0 and res["ok"] is True and res["mfma_f32_exact"] is True
            and res["hbm_gbps"] > 2000 and res["bf16_tflops"] > 500 and res["msg"] == "ok")


CLEAN_CHILD = """
import json
from cro_amd.nodeops.probe import run_probe
print(json.dumps([run_probe(0) for _ in range(20)]))  # the first sets the context up
"""


def test_twenty_consecutive_calls_are_clean():
    """The stream, the events and the pinned tile are reused call after call."""
    _require_gpu()
    results = _child(CLEAN_CHILD, timeout=120)
    assert len(results) == 20
    for i, res in enumerate(results):
        assert _healthy(res), (i, res)


def test_selftest_never_touches_the_cached_expected_tile():
    """Self-test calls flip a bit of their own copy of the expected tile: each
    fails, and the clean call after each passes against the cached one."""
    _require_gpu()
    from cro_amd.nodeops.probe import run_probe

    assert _healthy(run_probe(0))
    for elem, bit in ((0, 0), (255, 31), (165, 29)):
        res = run_probe(0, selftest_mode=1, selftest_elem=elem, selftest_bit=bit)
        assert res["rc"] == -2 and res["ok"] is False and res["mfma_f32_exact"] is False, res
        assert "f32 MFMA mismatch" in res["msg"], res
        res = run_probe(0)
        assert _healthy(res), (elem, bit, res)


def test_poisoned_tile_fails_when_the_check_kernel_did_not_run():
    """Directly after a call that left a good tile on the device, a call
    without the check kernel must not pass on it."""
    _require_gpu()
    from cro_amd.nodeops.probe import run_probe, run_probe_windows

    assert _healthy(run_probe(0))
    res = run_probe_windows(0, skip_check_launch=1)
    assert res["rc"] == -2 and res["ok"] is False and res["mfma_f32_exact"] is False, res
    assert "f32 MFMA mismatch" in res["msg"], res
    assert res["hbm_gbps"] > 0 and res["bf16_tflops"] > 0  # the rest of the pipeline ran
    assert _healthy(run_probe(0))


def test_smallest_and_parent_windows_and_argument_bounds():
    _require_gpu()
    from cro_amd.nodeops.probe import run_probe_windows

    for launches, iters in ((1, 256), (8, 2048)):
        res = run_probe_windows(0, copy_launches=launches, bf16_iters=iters)
        assert _healthy(res), (launches, iters, res)
    assert _healthy(run_probe_windows(0))  # zeros: the library's defaults
    assert _healthy(run_probe_windows(0, copy_launches=64, bf16_iters=256))  # the limit itself
    for opts in (
        {"copy_launches": 65},
        {"copy_launches": -1},
        {"bf16_iters": 65537},
        {"bf16_iters": -1},
        {"skip_check_launch": -1},
        {"skip_check_launch": 2},
    ):
        res = run_probe_windows(0, **opts)
        assert res["rc"] == -1 and res["ok"] is False, (opts, res)
        assert res["msg"].startswith("bad argument: "), (opts, res)
        assert res["hbm_gbps"] == 0.0  # refused before anything ran


EVENT_TIMES_CHILD = """
import json, time
from cro_amd.nodeops.probe import run_probe
run_probe(0)  # sets the context up
out = []
for _ in range(3):
    t0 = time.perf_counter()
    res = run_probe(0)
    res["host_ms"] = (time.perf_counter() - t0) * 1e3
    out.append(res)
print(json.dumps(out))
"""


def test_section_times_are_device_times_within_the_calls_wall():
    """Each section's time comes from its own pair of events: positive, and
    together no longer than the host saw the whole call take."""
    _require_gpu()
    for res in _child(EVENT_TIMES_CHILD, timeout=120):
        assert _healthy(res), res
        sections = [res["t_mfma_ms"], res["t_bw_ms"], res["t_bf16_ms"]]
        assert all(t > 0 for t in sections), res
        assert res["t_setup_ms"] >= 0, res
        assert sum(sections) <= res["host_ms"], res


SELFCHECK_CHILD = """
import json
from cro_amd.nodeops.probe import bw_selfcheck, run_probe_windows
before = bw_selfcheck(0)  # this call sets the cached context up
probe = run_probe_windows(0, copy_launches=1, bf16_iters=256)
print(json.dumps({"before": before, "probe": probe, "after": bw_selfcheck(0)}))
"""


def test_credited_copy_launch_still_writes_every_byte():
    """The self-check and the probe share the cached buffers and the stream
    under one mutex: all 256 MiB of dst arrive before and after a probe."""
    _require_gpu()
    out = _child(SELFCHECK_CHILD, timeout=120)
    assert out["before"] == NONE_BAD, out["before"]
    assert _healthy(out["probe"]), out["probe"]
    assert out["after"] == NONE_BAD, out["after"]
