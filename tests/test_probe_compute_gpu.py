"""GPU-marked tests of the compute-coverage probe stage on a real MI355X.

Every comparison is bit-exact: integer data on the i8 and bf16 matrix pipes,
the fmaf chain on the f32 pipe, the address pattern in LDS.  Detection and
localisation are shown with the stage's self-test modes, which alter one bit
of an expected value (mode 1) or of a computed value on the waves of one CU
(mode 2) — data mismatches only; nothing on the GPU is provoked.

Shapes: the lane-map tiles use one K step and three (accumulation); the clean
runs cross the grid sizes 1 (four records), 8, one workgroup per CU and 44
more than that (more workgroups than CUs) with LDS sizes of 1024 bytes (64
vectors: fewer than the 256 threads), 4096 + 16 (thread 0 takes a second
trip) and 163840 (a CU's whole LDS).
"""

import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_LDS = 163840
TEST_BITS = {"mfma_f32": 1, "mfma_i8": 2, "mfma_bf16": 4, "lds": 8}
BAD_COUNTS = ("bad_f32", "bad_i8", "bad_bf16", "bad_lds")


def _require_gpu():
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU (KFD) on this host")


_cache = {}


def _clean_default():
    """One clean run at defaults with its records, shared and read-only."""
    from cro_amd.nodeops.probe import run_compute_records

    if "clean" not in _cache:
        res, records = run_compute_records(0)
        records.setflags(write=False)
        _cache["clean"] = (res, records)
    return _cache["clean"]


def _keys(records):
    from cro_amd.nodeops.probe import cu_key

    return cu_key(records["xcc_id"].astype(np.int64), records["hw_id"].astype(np.int64))


# -- lane maps ----------------------------------------------------------------------


def _asymmetric_ints(rng, shape, lo, hi):
    m = rng.integers(lo, hi + 1, size=shape)
    n = min(shape)
    assert not np.array_equal(m[:n, :n], m[:n, :n].T)
    return m


@pytest.mark.parametrize("k", [64, 192])
def test_i8_lane_map_bit_exact(k):
    _require_gpu()
    from cro_amd.nodeops.probe import mfma_tile

    rng = np.random.default_rng(1000 + k)
    a = _asymmetric_ints(rng, (16, k), -9, 9).astype(np.int8)
    b = _asymmetric_ints(rng, (k, 16), -9, 9).astype(np.int8)
    got = mfma_tile(0, "i8", a, b)
    want = a.astype(np.int32) @ b.astype(np.int32)
    assert got.dtype == np.int32 and np.array_equal(got, want)


def test_i8_lane_map_int8_extremes():
    _require_gpu()
    from cro_amd.nodeops.probe import mfma_tile

    rng = np.random.default_rng(7)
    a = rng.integers(-128, 128, size=(16, 64)).astype(np.int8)
    b = rng.integers(-128, 128, size=(64, 16)).astype(np.int8)
    a[3, :4] = (-128, 127, -128, 127)
    b[:4, 5] = (-128, 127, 127, -128)  # (-128)^2, 127^2 and both mixed products
    got = mfma_tile(0, "i8", a, b)
    assert np.array_equal(got, a.astype(np.int32) @ b.astype(np.int32))
    # a row and a column of nothing but -128: the largest sum of one K step
    a[:] = -128
    b[:] = -128
    assert np.array_equal(mfma_tile(0, "i8", a, b), np.full((16, 16), 64 * 128 * 128))


@pytest.mark.parametrize("k", [16, 48])
def test_bf16_lane_map_bit_exact(k):
    _require_gpu()
    from cro_amd.nodeops.probe import mfma_tile

    rng = np.random.default_rng(2000 + k)
    a = _asymmetric_ints(rng, (32, k), -8, 8)
    b = _asymmetric_ints(rng, (k, 32), -8, 8)
    got = mfma_tile(0, "bf16", a.astype(np.float32), b.astype(np.float32))
    want = (a @ b).astype(np.float32)  # integers <= 48 * 64: exact in f32
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_mfma_tile_rejects_bad_k():
    _require_gpu()
    from cro_amd.nodeops.probe import mfma_tile

    with pytest.raises(RuntimeError):
        mfma_tile(0, "i8", np.zeros((16, 32), np.int8), np.zeros((32, 16), np.int8))
    with pytest.raises(RuntimeError):
        mfma_tile(0, "bf16", np.zeros((32, 8), np.float32), np.zeros((8, 32), np.float32))


def test_expected_tiles_match_the_raw_tile_entry():
    """The stage's own i8 and bf16 inputs through the raw entry give the
    numpy tiles the kernel is compared against."""
    _require_gpu()
    from cro_amd.nodeops.probe import compute_expected_tiles, compute_inputs, mfma_tile

    inputs, tiles = compute_inputs(0), compute_expected_tiles(0)
    assert np.array_equal(mfma_tile(0, "i8", *inputs["i8"]), tiles["i8"])
    a16, b16 = inputs["bf16"]
    got = mfma_tile(0, "bf16", a16.astype(np.float32), b16.astype(np.float32))
    assert np.array_equal(got.view(np.uint32), tiles["bf16"].view(np.uint32))


# -- clean runs ---------------------------------------------------------------------


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("lds_bytes", [1024, 4096 + 16, FULL_LDS])
@pytest.mark.parametrize("grid", ["1", "8", "default", "default+44"])
def test_clean_run(grid, lds_bytes, iters):
    _require_gpu()
    from cro_amd.nodeops.probe import decode_location, run_compute_records

    cus = _clean_default()[0]["cus_expected"]
    blocks = {"1": 1, "8": 8, "default": 0, "default+44": cus + 44}[grid]
    res, records = run_compute_records(0, grid_blocks=blocks, lds_bytes=lds_bytes, iters=iters)
    want_blocks = blocks or cus
    assert res["ok"] is True and res["rc"] == 0 and res["msg"] == "ok", res
    assert res["failed_test"] == "" and res["waves_bad"] == 0 and res["cus_bad"] == 0, res
    for name in BAD_COUNTS:
        assert res[name] == 0, (name, res)
    assert (res["grid_blocks"], res["lds_bytes"], res["iters"]) == (want_blocks, lds_bytes, iters)
    assert 1 <= res["rounds"] <= 4
    assert res["waves_run"] == 4 * want_blocks * res["rounds"], res
    assert len(records) == res["waves_run"]
    assert 1 <= res["cus_seen"] <= res["cus_expected"] == cus, res
    assert res["cus_seen"] <= res["simds_seen"] <= 4 * res["cus_seen"], res
    assert res["first_bad_index"] == -1 and res["first_bad_round"] == -1, res
    assert np.all(records["valid"] == 1) and not records["fail_mask"].any()
    assert not records["n_bad"].any() and np.all(records["first_bad"] == 0xFFFFFFFF)
    loc = decode_location(records["xcc_id"], records["hw_id"])
    assert loc["simd"].min() >= 0 and loc["simd"].max() <= 3
    assert loc["xcd"].max() <= 7
    assert res["gpu_ms"] > 0 and res["t_total_ms"] >= res["gpu_ms"]


@pytest.mark.parametrize(
    "opts",
    [{"lds_bytes": 1000}, {"lds_bytes": FULL_LDS + 16}, {"lds_bytes": -16}, {"grid_blocks": -1},
     {"iters": -1}, {"max_rounds": -1}, {"min_cu_fraction": 1.5},
     {"selftest_mode": 3}, {"selftest_mode": 1, "selftest_test": 4},
     {"selftest_mode": 1, "selftest_test": 0, "selftest_elem": 256},
     {"selftest_mode": 1, "selftest_test": 2, "selftest_elem": 1024},
     {"selftest_mode": 1, "selftest_test": 3, "selftest_elem": 256, "lds_bytes": 1024},
     {"selftest_mode": 2, "selftest_test": 1, "selftest_bit": 32}],
)
def test_bad_arguments_are_refused(opts):
    _require_gpu()
    from cro_amd.nodeops.probe import run_compute

    res = run_compute(0, **opts)
    assert res["ok"] is False and res["rc"] == -1 and res["rounds"] == 0, res
    assert res["msg"].startswith("bad argument"), res


def test_coverage_floor_gates_only_when_set():
    """Eight workgroups cannot reach every CU: reported, and refused only
    under a floor."""
    _require_gpu()
    from cro_amd.nodeops.probe import run_compute

    free = run_compute(0, grid_blocks=8, iters=1, max_rounds=1)
    assert free["ok"] is True and free["cus_seen"] <= 8 < free["cus_expected"], free
    floored = run_compute(0, grid_blocks=8, iters=1, max_rounds=1, min_cu_fraction=0.5)
    assert floored["ok"] is False and floored["rc"] == -31, floored
    assert floored["waves_bad"] == 0 and floored["failed_test"] == "", floored
    assert "below the floor" in floored["msg"]


# -- coverage -------------------------------------------------------------------------


def test_default_run_covers_every_cu_and_simd():
    """The point of the stage, and the check of the HW_ID field positions:
    as many distinct (XCD, SE, SH, CU) keys as the device has CUs, each with
    exactly the SIMD ids 0..3, on all eight XCDs."""
    _require_gpu()
    from cro_amd.nodeops.probe import decode_location

    res, records = _clean_default()
    print("coverage at defaults:", {k: res[k] for k in (
        "cus_expected", "cus_seen", "xcds_seen", "simds_seen", "rounds", "gpu_ms", "t_total_ms")})
    assert res["ok"] is True, res
    assert res["cus_seen"] == res["cus_expected"], res
    assert res["xcds_seen"] == 8, res
    assert res["simds_seen"] == 4 * res["cus_seen"], res
    keys = _keys(records)
    simd = decode_location(records["xcc_id"], records["hw_id"])["simd"]
    assert np.unique(keys).size == res["cus_expected"]
    for key in np.unique(keys):
        assert sorted(set(simd[keys == key].tolist())) == [0, 1, 2, 3], hex(int(key))
    per_xcd = np.bincount(np.unique(keys) >> 16, minlength=8)
    assert per_xcd.tolist() == [res["cus_expected"] // 8] * 8


# -- self-test mode 1: one bit of an expected value ------------------------------------

# lane >= 32 (the upper half of the wave) and a high bit:
#   f32 / i8 16x16: element row * 16 + col is held by lane 16 * (row // 4) + col
#   bf16 32x32: element row * 32 + col by lane 32 * ((row // 4) % 2) + col
#   lds: word w belongs to vector w // 4, checked by lane (w // 4) % 64
MODE1 = [
    ("mfma_f32", 10 * 16 + 5, 29),   # lane 37, register 2
    ("mfma_i8", 13 * 16 + 2, 31),    # lane 50, register 1
    ("mfma_bf16", 21 * 32 + 13, 30),  # lane 45, register 9
    ("lds", (40 + 3 * 256) * 4 + 2, 31),  # wave 0, lane 40, fourth trip, word 2
]


@pytest.mark.parametrize("test,elem,bit", MODE1)
def test_selftest_expected_bit_is_flagged_by_every_wave(test, elem, bit):
    _require_gpu()
    from cro_amd.nodeops.probe import decode_location, run_compute_records

    iters = 2
    res, records = run_compute_records(0, iters=iters, selftest_mode=1, selftest_test=test,
                                       selftest_elem=elem, selftest_bit=bit)
    assert res["ok"] is False and res["rc"] == -30, res
    assert res["rounds"] == 1  # a mismatch ends the run
    assert res["failed_test"] == test and res["first_fail_mask"] == TEST_BITS[test], res
    assert res["first_bad"] == elem and res["bits_bad"] == 1 << bit, res
    assert res["waves_bad"] == res["waves_run"] == len(records) == 4 * res["grid_blocks"], res
    assert res["cus_bad"] == res["cus_seen"] and res["n_bad_cu_keys"] == 8, res
    for name in BAD_COUNTS:
        want = res["waves_run"] if name == "bad_" + test.replace("mfma_", "") else 0
        assert res[name] == want, (name, res)
    assert (res["first_bad_index"], res["first_bad_round"], res["first_bad_record"]) == (0, 0, 0)
    loc = decode_location(int(records["xcc_id"][0]), int(records["hw_id"][0]))
    assert {k: res[k] for k in ("xcd", "se", "sh", "cu", "simd")} == {
        k: loc[k] for k in ("xcd", "se", "sh", "cu", "simd")}
    assert f"compute mismatch in {test} at xcd={loc['xcd']} " in res["msg"]
    # every wave: only this test, this element, this bit
    assert np.all(records["fail_mask"] == TEST_BITS[test])
    assert np.all(records["bits_bad"] == 1 << bit)
    if test == "lds":
        # the flip is repeated at the same lane and trip of each wave
        wave = np.arange(len(records)) % 4
        assert np.array_equal(records["first_bad"], elem + wave * 64 * 4)
        assert np.all(records["n_bad"] == 2 * iters)  # pattern and complement
    else:
        assert np.all(records["first_bad"] == elem)
        assert np.all(records["n_bad"] == iters)


# -- self-test mode 2: one bit of a computed value on one CU ---------------------------


@pytest.mark.parametrize("test,elem,bit", MODE1)
def test_selftest_computed_bit_is_located_on_its_cu(test, elem, bit):
    _require_gpu()
    from cro_amd.nodeops.probe import decode_cu_key, decode_location, run_compute_records

    clean = _clean_default()[1]
    key = int(_keys(clean)[len(clean) // 2 + 1])
    res, records = run_compute_records(0, iters=1, selftest_mode=2, selftest_test=test,
                                       selftest_elem=elem, selftest_bit=bit, selftest_key=key)
    on_cu = _keys(records) == key
    flagged = records["fail_mask"] != 0
    assert on_cu.any(), "the chosen CU ran no workgroup in this run"
    assert np.array_equal(flagged, on_cu)  # exactly those waves, and all of them
    assert on_cu.sum() % 4 == 0
    assert res["ok"] is False and res["rc"] == -30 and res["failed_test"] == test, res
    assert res["cus_bad"] == 1 and res["bad_cu_keys"] == [key], res
    assert res["waves_bad"] == int(on_cu.sum()), res
    assert res["bits_bad"] == 1 << bit, res
    first = int(np.flatnonzero(on_cu)[0])
    assert res["first_bad_index"] == first
    want = decode_cu_key(key)
    assert {k: res[k] for k in ("xcd", "se", "sh", "cu")} == want, res
    assert res["simd"] == decode_location(0, int(records["hw_id"][first]))["simd"]
    assert np.all(records["fail_mask"][on_cu] == TEST_BITS[test])
    assert np.all(records["bits_bad"][on_cu] == 1 << bit)
    if test != "lds":
        assert np.all(records["first_bad"][on_cu] == elem)
    # a key no CU has: nothing is flagged
    res, records = run_compute_records(0, iters=1, selftest_mode=2, selftest_test=test,
                                       selftest_elem=elem, selftest_bit=bit,
                                       selftest_key=key | (0xF << 20))
    assert res["ok"] is True and not records["fail_mask"].any(), res


# -- croagent, lifecycle -----------------------------------------------------------------


def test_croagent_probe_compute():
    _require_gpu()
    from cro_amd.nodeops.probe import CroComputeResult

    agent = os.path.join(REPO, "cro_amd", "agent", "croagent")
    assert os.path.exists(agent), "croagent not built (python -m cro_amd.hip.build)"
    argv = [agent, "probe", "--device", "0"]
    run = subprocess.run(argv + ["--compute"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = json.loads(run.stdout)
    comp = out["compute"]
    assert out["ok"] is True and comp["ok"] is True and "integrity" not in out, out
    assert comp["waves_bad"] == 0 and comp["xcds_seen"] == 8, comp
    assert comp["cus_seen"] == comp["cus_expected"], comp
    # the same keys as run_compute's dict
    want = {name for name, _ in CroComputeResult._fields_} - {"reserved"}
    assert set(comp) == want
    floored = subprocess.run(argv + ["--compute", "--compute-min-cu-fraction", "0.5"],
                             capture_output=True, text=True, timeout=120)
    assert floored.returncode == 0 and json.loads(floored.stdout)["compute"]["ok"] is True
    quick = subprocess.run(argv, capture_output=True, text=True, timeout=120)
    assert quick.returncode == 0, quick.stdout + quick.stderr
    assert "compute" not in json.loads(quick.stdout)


def test_compute_lifecycle_real_node_path():
    """One attach→detach with quick + compute as the node-ops hook."""
    _require_gpu()
    from cro_amd.api.v1alpha1.types import Event
    from cro_amd.bench_harness import attach_detach_cycle, build_local_stack
    from cro_amd.nodeops.probe import make_probe_fn

    cdi_dir = os.path.join(os.environ.get("TMPDIR", "/tmp"), "cro-cdi-computetest")
    stack = build_local_stack(node_name="computetest", use_gpu=True, gpu_index=0,
                              cdi_dir=cdi_dir)
    stack.ops.probe_fn = make_probe_fn("quick", compute=True)
    stack.mgr.start()
    try:
        attach_detach_cycle(stack, "compute-e2e", size=1, timeout=180)
        assert stack.ops.cdi.devices("computetest") == []
        stack.mgr.recorder.flush()
        online = [e for e in stack.mgr.client.list(Event) if e.reason == "Online"]
        assert online and "; compute: " in online[-1].message, online
        assert " CUs, " in online[-1].message and " SIMDs, " in online[-1].message
    finally:
        stack.mgr.stop()
