"""GPU-marked tests of the quick probe's three kernels, its gates and its
locking on a real MI355X (cro_amd/hip/probe.hip).

Every comparison is bit-exact.  The copy kernel moves an address-dependent
pattern, so a wrong index shows; the bf16 rate kernel's sums are multiples of
1/512 below 2^15, exact in float32 in any order (tests/test_probe_quick.py
asserts the bound); the f32 tile is compared with the k-ordered fmaf chain,
whose numpy form the same file proves against a true ``fmaf`` for each input
used here.  The gates fire through options alone: a floor no device reaches,
or one flipped bit of the host's expected tile.  Nothing on the GPU is
provoked.
"""

import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_probe_quick import f32_cases

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_CASES = f32_cases()


def _require_gpu():
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU (KFD) on this host")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _child(code, timeout):
    """Run ``code`` in a fresh interpreter with a time limit of its own; the
    last line it prints is JSON."""
    proc = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True,
                          text=True, timeout=timeout)
    assert proc.returncode == 0, (proc.returncode, proc.stdout[-2000:], proc.stderr[-2000:])
    return json.loads(proc.stdout.strip().splitlines()[-1])


# -- copy kernel ------------------------------------------------------------------------

COPY_CASES = [
    (1, 1), (1, 255), (1, 256),  # single workgroup, up to one full block
    (1, 257),  # one thread takes a second trip
    (2, 512), (2, 513),  # two workgroups, exact and one over
    (3, 3 * 256 * 4 + 5),  # uneven trip counts
    (8192, 8192 * 256 + 5),  # the probe's own grid, 32 MiB, five threads on a second trip
]


@pytest.mark.parametrize("grid,n4", COPY_CASES)
def test_copy_kernel_exact(grid, n4):
    _require_gpu()
    from cro_amd.nodeops.probe import copy_vectors, pattern_words

    src = pattern_words(0xFFFFFF00, 4 * n4, seed=grid, invert=False)
    keep = src.copy()
    got = copy_vectors(0, src, grid)
    assert np.array_equal(src, keep)
    bad = np.flatnonzero(got["dst"] != src)
    assert bad.size == 0, (f"{bad.size} of {src.size} words differ, first at word {bad[0]} "
                           f"(vector {bad[0] // 4})")
    assert got["guard_ok"], "the copy wrote past n4 vectors"
    assert got["src_unchanged"], "the copy changed its source"


def test_copy_refuses_bad_arguments():
    _require_gpu()
    from cro_amd.nodeops.probe import copy_vectors, load_library

    with pytest.raises(RuntimeError, match="rc=-10"):
        copy_vectors(0, np.zeros(0, np.uint32), 1)  # n4 = 0
    with pytest.raises(RuntimeError, match="rc=-10"):
        copy_vectors(0, np.zeros(4, np.uint32), 0)
    with pytest.raises(RuntimeError, match="rc=-10"):
        copy_vectors(0, np.zeros(4, np.uint32), (1 << 16) + 1)
    lib = load_library(required=True)
    ok = ctypes.c_int(7)
    buf = np.zeros(4, np.uint32)
    assert lib.cro_probe_copy(0, None, 1, 1, buf.ctypes.data, ctypes.byref(ok)) == -10
    assert lib.cro_probe_copy(0, buf.ctypes.data, 1, 1, None, ctypes.byref(ok)) == -10
    assert lib.cro_probe_copy(0, buf.ctypes.data, 1, 1, buf.ctypes.data, None) == -10
    assert lib.cro_probe_copy(0, buf.ctypes.data, (1 << 24) + 1, 1, buf.ctypes.data,
                              ctypes.byref(ok)) == -10


SELFCHECK_CHILD = """
import json
from cro_amd.nodeops.probe import bw_selfcheck, run_probe
fresh = bw_selfcheck(0)  # this call sets the cached context up
probe = run_probe(0)
print(json.dumps({"fresh": fresh, "probe": probe, "after": bw_selfcheck(0)}))
"""


def test_probes_own_copy_launch_writes_every_byte():
    """hbm_gbps credits 2 x 256 MiB per launch: all 256 MiB of dst arrive, on
    a context the self-check set up itself and again after a probe."""
    _require_gpu()
    out = _child(SELFCHECK_CHILD, timeout=120)
    assert out["fresh"] == {"n_bad": 0, "first_bad": 2 ** 64 - 1}, out["fresh"]
    assert out["probe"]["ok"] and out["probe"]["mfma_f32_exact"], out["probe"]
    assert out["after"] == {"n_bad": 0, "first_bad": 2 ** 64 - 1}, out["after"]


# -- bf16 rate kernel -----------------------------------------------------------------------


@pytest.mark.parametrize("iters", [1, 3, 64])
@pytest.mark.parametrize("blocks", [1, 3])
def test_bf16_sink_exact(blocks, iters):
    _require_gpu()
    from cro_amd.nodeops.probe import bf16_sink, quick_bf16_lane_sums

    lanes = quick_bf16_lane_sums(iters)  # float64, exact
    want = np.tile(lanes, 4 * blocks).astype(np.float32)  # four waves per block
    assert np.array_equal(want.astype(np.float64), np.tile(lanes, 4 * blocks))
    got = bf16_sink(0, blocks, iters, all_lanes=True)
    assert got.shape == (blocks * 256,)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (f"{bad.size} of {got.size} lane sums differ, first: thread "
                           f"{bad[0]} got {got[bad[0]]!r} want {want[bad[0]]!r}")
    # the probe's own variant: thread 0 of each block
    lane0 = bf16_sink(0, blocks, iters, all_lanes=False)
    assert lane0.shape == (blocks,)
    assert np.array_equal(_bits(lane0), _bits(np.full(blocks, lanes[0], dtype=np.float32)))


def test_bf16_sink_zero_iterations_and_bad_arguments():
    _require_gpu()
    from cro_amd.nodeops.probe import bf16_sink

    # the buffer is preset to NaNs: zeros mean every thread stored
    assert np.array_equal(_bits(bf16_sink(0, 3, 0, all_lanes=True)), np.zeros(768, np.uint32))
    assert np.array_equal(_bits(bf16_sink(0, 3, 0, all_lanes=False)), np.zeros(3, np.uint32))
    for blocks, iters in ((0, 1), (1025, 1), (1, -1), (1, (1 << 16) + 1)):
        with pytest.raises(RuntimeError, match="rc=-10"):
            bf16_sink(0, blocks, iters, all_lanes=True)


# -- f32 tile ---------------------------------------------------------------------------------


def _describe_f32_mismatch(name, got, want):
    bad = np.argwhere(_bits(got) != _bits(want))
    xor = np.bitwise_or.reduce((_bits(got) ^ _bits(want)).ravel())
    r, c = bad[0]
    return (f"{name}: {len(bad)} of 256 elements differ, bits 0x{xor:08x}; first [{r}][{c}] "
            f"got 0x{_bits(got)[r, c]:08x} want 0x{_bits(want)[r, c]:08x}")


@pytest.mark.parametrize("name", sorted(F32_CASES))
def test_mfma_f32_tile_is_bitwise_the_fmaf_chain(name):
    """The claim the probe's hard gate rests on (probe.hip): the f32 matrix
    pipe equals a k-ordered fmaf chain bit for bit, subnormals un-flushed,
    signed zeros included.  One K step, two, three, the probe's 64 and long
    chains; integers for the lane map; subnormals, zeros and cancellation."""
    _require_gpu()
    from cro_amd.nodeops.probe import fmaf_chain, mfma_f32_tile

    a, b = F32_CASES[name]
    want, ties = fmaf_chain(a, b)
    assert ties == 0  # the numpy form is the true chain (tests/test_probe_quick.py)
    got = mfma_f32_tile(0, a, b)
    assert got.dtype == np.float32 and got.shape == (16, 16)
    assert np.array_equal(_bits(got), _bits(want)), _describe_f32_mismatch(name, got, want)


def test_mfma_f32_tile_refuses_bad_arguments():
    _require_gpu()
    from cro_amd.nodeops.probe import load_library, mfma_f32_tile

    for k in (6, 0, 4100):
        with pytest.raises(RuntimeError, match="rc=-10"):
            mfma_f32_tile(0, np.zeros((16, k), np.float32), np.zeros((k, 16), np.float32))
    lib = load_library(required=True)
    buf = np.zeros(256, np.float32)
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.cro_probe_mfma_f32(0, None, p, p, 4) == -10
    assert lib.cro_probe_mfma_f32(0, p, None, p, 4) == -10
    assert lib.cro_probe_mfma_f32(0, p, p, None, 4) == -10
    assert lib.cro_probe_mfma_f32(0, p, p, p, 4096 + 4) == -10


# -- gates ------------------------------------------------------------------------------------

SELFTEST = {"selftest_mode": 1, "selftest_elem": 10 * 16 + 5, "selftest_bit": 29}


def test_gates_fire_in_order_and_leave_the_probe_clean():
    _require_gpu()
    from cro_amd.nodeops.probe import run_probe

    res = run_probe(0, hbm_floor_gbps=1e9)
    assert res["rc"] == -3 and res["ok"] is False and res["mfma_f32_exact"] is True, res
    assert "HBM bandwidth" in res["msg"] and "below floor" in res["msg"], res
    assert res["hbm_gbps"] > 0 and res["bf16_tflops"] > 0  # measured all the same

    res = run_probe(0, bf16_floor_tflops=1e9)
    assert res["rc"] == -4 and res["ok"] is False and res["mfma_f32_exact"] is True, res
    assert "bf16 MFMA" in res["msg"] and "below floor" in res["msg"], res

    res = run_probe(0, **SELFTEST)
    assert res["rc"] == -2 and res["ok"] is False and res["mfma_f32_exact"] is False, res
    assert "f32 MFMA mismatch" in res["msg"], res

    # the exact gate comes first, then bandwidth, then the matrix rate
    res = run_probe(0, hbm_floor_gbps=1e9, bf16_floor_tflops=1e9, **SELFTEST)
    assert res["rc"] == -2 and res["mfma_f32_exact"] is False, res
    res = run_probe(0, hbm_floor_gbps=1e9, bf16_floor_tflops=1e9)
    assert res["rc"] == -3, res

    # floors a healthy device clears change nothing, and nothing sticks
    res = run_probe(0, hbm_floor_gbps=2000, bf16_floor_tflops=500)
    assert res["rc"] == 0 and res["ok"] is True and res["msg"] == "ok", res
    res = run_probe(0)
    assert res["rc"] == 0 and res["ok"] is True and res["mfma_f32_exact"] is True, res
    assert res["msg"] == "ok"


def test_every_selftest_bit_and_corner_element_trips_the_exact_gate():
    """The compare looks at all 256 elements and all 32 bits of each."""
    _require_gpu()
    from cro_amd.nodeops.probe import run_probe

    for elem, bit in ((0, 0), (255, 31), (15, 23), (240, 1)):
        res = run_probe(0, selftest_mode=1, selftest_elem=elem, selftest_bit=bit)
        assert res["rc"] == -2 and res["mfma_f32_exact"] is False, (elem, bit, res)


def test_device_out_of_range_and_bad_options():
    _require_gpu()
    from cro_amd.nodeops.probe import device_count, run_probe

    count = device_count()
    assert count >= 1
    for device in (-1, count):
        for opts in ({}, {"hbm_floor_gbps": 600.0}):
            res = run_probe(device, **opts)
            assert res["rc"] == -1 and res["ok"] is False, res
            assert "out of range" in res["msg"], res
    for opts in (
        {"selftest_mode": 1, "selftest_elem": 256},
        {"selftest_mode": 1, "selftest_bit": 32},
        {"selftest_mode": 1, "selftest_bit": -1},
        {"selftest_mode": 2},
        {"selftest_mode": -1},
        {"hbm_floor_gbps": -1.0},
        {"bf16_floor_tflops": -0.5},
        {"hbm_floor_gbps": float("nan")},
    ):
        res = run_probe(0, **opts)
        assert res["rc"] == -1 and res["ok"] is False, (opts, res)
        assert res["msg"].startswith("bad argument: "), (opts, res)
        assert res["hbm_gbps"] == 0.0  # refused before anything ran


# -- concurrency --------------------------------------------------------------------------------

CONCURRENT_CHILD = """
import json, threading
from cro_amd.nodeops.probe import load_library, run_probe
load_library(required=True)
barrier = threading.Barrier(4)
results = [None] * 4
def worker(i):
    barrier.wait(timeout=60)
    results[i] = [run_probe(0) for _ in range(3)]  # the first of them sets the context up
threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
for t in threads: t.start()
for t in threads: t.join()
print(json.dumps([r for per in results for r in (per or [])]))
"""


def test_concurrent_probes_on_one_device_are_serialised():
    """Four reconcile workers attach on one device at once (ctypes releases
    the GIL): one context, and every rate computed from its own events."""
    _require_gpu()
    results = _child(CONCURRENT_CHILD, timeout=180)
    assert len(results) == 12
    for res in results:
        assert res["ok"] and res["rc"] == 0 and res["mfma_f32_exact"], res
        # the floors of test_probe_extension_loads_and_passes (tests/test_gpu.py)
        assert res["hbm_gbps"] > 2000 and res["bf16_tflops"] > 500, res
    assert len({res["vram_free"] for res in results}) == 1, [r["vram_free"] for r in results]
    assert len({res["vram_total"] for res in results}) == 1
