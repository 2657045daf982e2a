"""GPU-marked tests of the matrix-format probe stage on a real MI355X.

Every comparison is bit-exact.  The lane, packing and scale maps written at
the head of cro_amd/hip/croformats.h are proved through cro_formats_tile,
which runs one wave of the stage's own product code on caller data: random
asymmetric data from each check's code set at one and at two instructions of
K, a one-hot sweep over every k of one instruction, one scale byte changed at
a time, every op_sel.  Detection and localisation of the stage are shown with
its self-test modes, which alter one bit of an expected value (mode 1) or of a
computed value on the waves of one CU (mode 2): data mismatches only; nothing
on the GPU is provoked.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cro_amd.nodeops import formats as F

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = list(range(len(F.FORMATS_TESTS)))
NAMES = list(F.FORMATS_TESTS)
SCALED = [i for i in TESTS if F.FORMATS_TABLE[i].scaled]
# the code of 1.0 in each operand format
ONE = {F.E4M3: 0x38, F.E5M2: 0x3C, F.E2M3: 0x08, F.E3M2: 0x0C, F.E2M1: 0x2, F.F16: 0x3C00}


def _require_gpu():
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU (KFD) on this host")


_cache = {}


def _inputs(idx, seed=0):
    """A check's inputs, shared and read-only."""
    if (idx, seed) not in _cache:
        inp = F.formats_inputs(idx, seed)
        for arr in inp.values():
            arr.setflags(write=False)
        _cache[idx, seed] = inp
    return _cache[idx, seed]


def _clean_default():
    """One clean run at defaults with its records, shared and read-only."""
    if "clean" not in _cache:
        res, records = F.run_formats_records(0)
        records.setflags(write=False)
        _cache["clean"] = (res, records)
    return _cache["clean"]


def _operands(idx, seed, k):
    """(codes or values for the tile entry, values) of both sides, first k columns."""
    t = F.FORMATS_TABLE[idx]
    inp = _inputs(idx, seed)
    key = "val" if t.fmt_a == F.F64 else "codes"
    return (inp[f"{key}_a"][:, :k], inp[f"{key}_b"][:, :k], inp["val_a"][:, :k],
            inp["val_b"][:, :k])


def _same_bits(got, want):
    want = np.asarray(want).astype(got.dtype)
    return np.array_equal(got.view(np.uint8), want.view(np.uint8))


# -- lane maps, one wave ---------------------------------------------------------------


@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("idx", TESTS, ids=NAMES)
def test_tile_random_data_matches_numpy_bit_for_bit(idx, steps):
    _require_gpu()
    t = F.FORMATS_TABLE[idx]
    for seed in (0, 5):
        k = steps * t.kstep
        ca, cb, va, vb = _operands(idx, seed, k)
        sa = sb = None
        if t.scaled:
            inp = _inputs(idx, seed)
            sa, sb = inp["scale_a"][:, : k // 32], inp["scale_b"][:, : k // 32]
        want = F.formats_product(va, vb, sa, sb)
        assert not np.array_equal(want, want.T)  # asymmetric: a swapped index shows
        got = F.formats_tile(0, idx, ca, cb, sa, sb, t.op_sel_a, t.op_sel_b)
        assert _same_bits(got, want), (t.name, seed, int((got != want).sum()))


@pytest.mark.parametrize("idx", TESTS, ids=NAMES)
def test_tile_one_hot_sweep_pins_every_k_of_one_instruction(idx):
    """A single 1.0 at A[r0][k0], for every k0, against a B of distinct values:
    row r0 of D is column k0 of B and every other row is zero.  For the scaled
    checks every K block has a scale of its own on both sides, so a k that the
    hardware takes from another block than the host shows; for fp6 the sweep
    walks the 6-bit fields across the byte boundaries."""
    _require_gpu()
    t = F.FORMATS_TABLE[idx]
    k, r0 = t.kstep, 5
    _, cb, _, vb = _operands(idx, 0, k)
    assert len({tuple(vb[:, j]) for j in range(k)}) == k  # the columns of B differ
    sa = sb = None
    wa = wb = np.ones((t.m, 1))
    if t.scaled:
        g = k // 32
        sa = (120 + (np.arange(t.m)[:, None] + np.arange(g)[None, :]) % 5).astype(np.uint8)
        sb = (131 + (np.arange(t.m)[:, None] + 2 * np.arange(g)[None, :]) % 7).astype(np.uint8)
        wa, wb = F.scale_value(sa), F.scale_value(sb)
    for k0 in range(k):
        if t.fmt_a == F.F64:
            ca = np.zeros((t.m, k))
            ca[r0, k0] = 1.0
        else:
            ca = np.zeros((t.m, k), np.uint16)
            ca[r0, k0] = ONE[t.fmt_a]
        got = F.formats_tile(0, idx, ca, cb, sa, sb)
        want = np.zeros((t.m, t.m))
        g0 = k0 // 32 if t.scaled else 0
        want[r0, :] = vb[:, k0] * wa[r0, g0] * wb[:, g0]
        # by value: float32 to float64 is exact, and a zero may have either sign
        assert np.array_equal(got.astype(np.float64), want), (t.name, k0)


def test_fp6_packing_crosses_byte_boundaries():
    """Host side of the sweep above: four 6-bit codes in three bytes."""
    packed = F.pack_codes(F.E2M3, np.array([[0x3F, 0x00, 0x15, 0x2A]], np.uint16))
    assert packed.tolist() == [[0x3F, 0x50, 0xA9]]


# -- scales -------------------------------------------------------------------------------


@pytest.mark.parametrize("idx", SCALED, ids=[NAMES[i] for i in SCALED])
def test_one_scale_byte_changes_exactly_its_row_or_column(idx):
    _require_gpu()
    t = F.FORMATS_TABLE[idx]
    k = 2 * t.kstep
    g = k // 32
    ca, cb, va, vb = _operands(idx, 0, k)
    sa0 = np.full((t.m, g), 127, np.uint8)
    base = F.formats_tile(0, idx, ca, cb, sa0, sa0).astype(np.float64)
    assert np.array_equal(base, F.formats_product(va, vb, sa0, sa0))
    for side, r, blk, byte in (("a", 3, 0, 129), ("a", t.m - 1, g - 1, 124),
                               ("b", 7, 1, 130), ("b", 0, g - 2, 125)):
        sa, sb = sa0.copy(), sa0.copy()
        (sa if side == "a" else sb)[r, blk] = byte
        got = F.formats_tile(0, idx, ca, cb, sa, sb).astype(np.float64)
        want = F.formats_product(va, vb, sa, sb)
        assert np.array_equal(got, want), (t.name, side, r, blk)
        changed = got != base
        line = changed[r, :] if side == "a" else changed[:, r]
        other = np.delete(changed, r, axis=0 if side == "a" else 1)
        assert line.any() and not other.any(), (t.name, side, r, blk)


@pytest.mark.parametrize("idx", SCALED, ids=[NAMES[i] for i in SCALED])
def test_each_op_sel_picks_its_own_byte(idx):
    """The kernel puts the scale in byte op_sel and three other valid scales
    in the other bytes: all sixteen selects give the same, right tile."""
    _require_gpu()
    t = F.FORMATS_TABLE[idx]
    k = t.kstep
    ca, cb, va, vb = _operands(idx, 0, k)
    inp = _inputs(idx, 0)
    sa, sb = inp["scale_a"][:, : k // 32], inp["scale_b"][:, : k // 32]
    want = F.formats_product(va, vb, sa, sb)
    for osa in range(4):
        for osb in range(4):
            got = F.formats_tile(0, idx, ca, cb, sa, sb, osa, osb)
            assert _same_bits(got, want), (t.name, osa, osb)


# -- f64 -----------------------------------------------------------------------------------


def test_f64_rows_land_in_lane_group_plus_four_r():
    """A = row number on the diagonal block, B = ones: D[r][c] = r + 1 in
    every column; with the f32 result map three of four rows would be wrong."""
    _require_gpu()
    a = np.zeros((16, 4))
    a[:, 0] = np.arange(1, 17)
    b = np.zeros((16, 4))
    b[:, 0] = 1.0 + np.arange(16) * 16.0
    got = F.formats_tile(0, "mfma_f64", a, b)
    assert np.array_equal(got, np.outer(a[:, 0], b[:, 0]))


# -- stage ---------------------------------------------------------------------------------


@pytest.mark.parametrize("seed", [0, 0xC0FFEE])
@pytest.mark.parametrize("iters", [1, 0])
@pytest.mark.parametrize("grid", [1, 2, 0])
def test_stage_is_clean(grid, iters, seed):
    _require_gpu()
    res, records = F.run_formats_records(0, grid_blocks=grid, iters=iters, seed=seed)
    assert res["ok"] is True and res["rc"] == 0 and res["msg"] == "ok", res
    assert res["waves_bad"] == 0 and res["first_fail_mask"] == 0, res
    assert all(res[f"bad_{name}"] == 0 for name in NAMES), res
    blocks = grid or res["cus_expected"]
    assert res["grid_blocks"] == blocks and res["waves_run"] == 4 * blocks * res["rounds"]
    assert res["iters"] == (iters or 64)  # the library default
    assert F.aggregate_formats_records(records) == {
        k: res[k] for k in F.aggregate_formats_records(records)}


def test_default_run_covers_every_cu_xcd_and_simd():
    _require_gpu()
    res, records = _clean_default()
    assert res["ok"] is True, res
    assert res["cus_seen"] == res["cus_expected"] > 0, res
    assert res["xcds_seen"] == 8 and res["simds_seen"] == 4 * res["cus_seen"], res
    assert np.all(records["valid"] == 1) and np.all(records["fail_mask"] == 0)


def test_coverage_floor_gates_only_when_set():
    _require_gpu()
    res = F.run_formats(0, grid_blocks=1, max_rounds=1)
    assert res["ok"] is True and res["cus_seen"] == 1, res
    res = F.run_formats(0, grid_blocks=1, max_rounds=1, min_cu_fraction=0.5)
    assert res["ok"] is False and res["rc"] == F.RC_COVERAGE and "below the floor" in res["msg"]


# -- self-test -----------------------------------------------------------------------------

MODE1 = [(idx, elem, bit) for idx in TESTS
         for elem in (0, F.FORMATS_TABLE[idx].elems - 1) for bit in (0, 31)]


@pytest.mark.parametrize("idx,elem,bit", MODE1)
def test_selftest_expected_bit_is_flagged_by_every_wave(idx, elem, bit):
    _require_gpu()
    res, records = F.run_formats_records(0, grid_blocks=3, iters=2, max_rounds=1,
                                         selftest_mode=1, selftest_test=idx,
                                         selftest_elem=elem, selftest_bit=bit)
    assert res["ok"] is False and res["rc"] == F.RC_MISMATCH, res
    assert res["failed_test"] == NAMES[idx] and NAMES[idx] in res["msg"], res
    assert res["waves_bad"] == res["waves_run"] == 12 and res[f"bad_{NAMES[idx]}"] == 12, res
    assert np.all(records["fail_mask"] == 1 << idx)
    assert np.all(records["first_bad"] == elem) and np.all(records["bits_bad"] == 1 << bit)
    assert np.all(records["n_bad"] == 2)  # one value, once per iteration


def test_selftest_computed_bit_is_located_on_its_cu():
    _require_gpu()
    _, clean = _clean_default()
    key = ((int(clean["xcc_id"][40]) & 0xF) << 16) | (int(clean["hw_id"][40]) & 0xFF00)
    for idx, elem, bit in ((1, 17, 3), (4, 1023, 30), (6, 255, 31)):
        res, records = F.run_formats_records(0, iters=1, selftest_mode=2, selftest_test=idx,
                                             selftest_elem=elem, selftest_bit=bit,
                                             selftest_key=key)
        assert res["ok"] is False and res["rc"] == F.RC_MISMATCH, res
        keys = ((records["xcc_id"].astype(np.int64) & 0xF) << 16) | (
            records["hw_id"].astype(np.int64) & 0xFF00)
        bad = records["fail_mask"] != 0
        assert np.array_equal(bad, keys == key) and int(bad.sum()) == 4, (idx, int(bad.sum()))
        assert np.all(records["first_bad"][bad] == elem)
        assert np.all(records["bits_bad"][bad] == 1 << bit)
        loc = {"xcd": key >> 16, "se": (key >> 13) & 7, "sh": (key >> 12) & 1,
               "cu": (key >> 8) & 0xF}
        assert {k: res[k] for k in loc} == loc and res["cus_bad"] == 1, res
        assert res["failed_test"] == NAMES[idx]


def test_the_lowest_failing_check_leads():
    """Two checks fail in every wave: the record and the result carry the
    element and bits of the one with the lowest mask bit, whichever of the two
    the options name first."""
    _require_gpu()
    for first, also, lead_elem in (("mx_fp4", "mfma_bf8", 10), ("mfma_bf8", "mx_fp4", 9)):
        res, records = F.run_formats_records(0, grid_blocks=2, iters=1, max_rounds=1,
                                             selftest_mode=1, selftest_test=first,
                                             selftest_also=also, selftest_elem=9,
                                             selftest_bit=4)
        assert res["rc"] == F.RC_MISMATCH and res["failed_test"] == "mfma_bf8", res
        assert res["bad_mfma_bf8"] == res["bad_mx_fp4"] == 8 and res["waves_bad"] == 8, res
        assert np.all(records["fail_mask"] == (1 << 2) | (1 << 5))
        assert np.all(records["n_bad"] == 2) and np.all(records["first_bad"] == lead_elem)
        assert res["first_bad"] == lead_elem and res["bits_bad"] == 1 << 4, res


# -- edges and lifecycle -------------------------------------------------------------------


@pytest.mark.parametrize("opts", [
    {"grid_blocks": -1}, {"grid_blocks": (1 << 16) + 1}, {"iters": -1}, {"max_rounds": 65},
    {"min_cu_fraction": 1.5}, {"min_cu_fraction": float("nan")}, {"selftest_mode": 3},
    {"selftest_mode": 1, "selftest_test": 7}, {"selftest_mode": 1, "selftest_elem": 256},
    {"selftest_mode": 1, "selftest_bit": 32},
    {"selftest_mode": 1, "selftest_test": 6, "selftest_bit": 64},
    {"selftest_also": "mfma_f16"}, {"selftest_mode": 1, "selftest_also": "mfma_f16"},
    {"selftest_mode": 2, "selftest_also": "mfma_fp8"},
])
def test_bad_options_are_refused(opts):
    _require_gpu()
    res = F.run_formats(0, **opts)
    assert res["ok"] is False and res["rc"] == -1 and "bad argument" in res["msg"], res


def test_tile_entry_refuses_bad_arguments():
    _require_gpu()
    ca = np.zeros((16, 48), np.uint16)
    with pytest.raises(RuntimeError):
        F.formats_tile(0, "mfma_fp8", ca, ca)  # K no multiple of 32
    ca = np.zeros((16, 32), np.uint16)
    with pytest.raises(RuntimeError):
        F.formats_tile(0, "mfma_fp8", ca, ca, op_sel_a=1)  # no scales to select


CONCURRENT_CHILD = r"""
import json, threading
from cro_amd.nodeops.formats import run_formats
results = [None] * 4
def work(i):
    results[i] = [run_formats(0, grid_blocks=8 + i, iters=1 + i, seed=100 + i, max_rounds=1)
                  for _ in range(3)]
threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
for t in threads: t.start()
for t in threads: t.join()
print(json.dumps(results))
"""


def test_concurrent_formats_stages_on_one_device_are_serialised():
    """Four threads on one device, each with a seed of its own: every call
    finds the tiles of its seed and reports its own options."""
    _require_gpu()
    proc = subprocess.run([sys.executable, "-c", CONCURRENT_CHILD], cwd=REPO,
                          capture_output=True, text=True, timeout=180)
    assert proc.returncode == 0, (proc.returncode, proc.stdout[-2000:], proc.stderr[-2000:])
    results = json.loads(proc.stdout.strip().splitlines()[-1])
    assert len(results) == 4
    for i, per_thread in enumerate(results):
        assert per_thread is not None and len(per_thread) == 3
        for res in per_thread:
            assert res["ok"] is True and res["rc"] == 0 and res["waves_bad"] == 0, (i, res)
            assert (res["grid_blocks"], res["iters"], res["rounds"]) == (8 + i, 1 + i, 1)
            assert res["waves_run"] == 4 * (8 + i), (i, res)


def test_croagent_probe_formats_key_order():
    _require_gpu()
    agent = os.path.join(REPO, "cro_amd", "agent", "croagent")
    assert os.path.exists(agent), "croagent not built (python -m cro_amd.hip.build)"
    argv = [agent, "probe", "--device", "0"]
    run = subprocess.run(argv + ["--compute", "--formats", "--deep", "--vram-mib", "64",
                                 "--link-mib", "16"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = json.loads(run.stdout)
    keys = list(out)
    assert keys[-3:] == ["compute", "formats", "integrity"], keys
    fmts = out["formats"]
    assert out["ok"] is True and fmts["ok"] is True and fmts["waves_bad"] == 0, out
    assert fmts["cus_seen"] == fmts["cus_expected"] and fmts["xcds_seen"] == 8, fmts
    # the same keys as run_formats' dict, in its order
    want = ["ok", "rc"] + [name for name, _ in F.CroFormatsResult._fields_
                           if name not in ("ok", "rc", "reserved")]
    assert list(fmts) == want
    quick = subprocess.run(argv, capture_output=True, text=True, timeout=120)
    assert quick.returncode == 0 and "formats" not in json.loads(quick.stdout)


def test_formats_lifecycle_real_node_path():
    """One attach→detach with quick + formats as the node-ops hook."""
    _require_gpu()
    from cro_amd.api.v1alpha1.types import Event
    from cro_amd.bench_harness import attach_detach_cycle, build_local_stack
    from cro_amd.nodeops.probe import make_probe_fn

    cdi_dir = os.path.join(os.environ.get("TMPDIR", "/tmp"), "cro-cdi-formatstest")
    stack = build_local_stack(node_name="formatstest", use_gpu=True, gpu_index=0,
                              cdi_dir=cdi_dir)
    stack.ops.probe_fn = make_probe_fn("quick", formats=True)
    stack.mgr.start()
    try:
        attach_detach_cycle(stack, "formats-e2e", size=1, timeout=180)
        assert stack.ops.cdi.devices("formatstest") == []
        stack.mgr.recorder.flush()
        online = [e for e in stack.mgr.client.list(Event) if e.reason == "Online"]
        assert online and "; formats: " in online[-1].message, online
        assert " CUs, " in online[-1].message and " SIMDs, " in online[-1].message
    finally:
        stack.mgr.stop()
