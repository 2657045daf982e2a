"""GPU tests of what the per-wave probe stages (compute coverage, matrix
formats, data movement) share on the host, for each of the three: the rounds
of one run, the bounded copy of the records to the caller and the end of the
run at a mismatch (round driver, cro_amd/hip/crohost.h).  Needs a real AMD GPU
(gfx950) and the built libraries."""

import ctypes
import os

import numpy as np
import pytest

from cro_amd.nodeops import formats as F
from cro_amd.nodeops import movement as M
from cro_amd.nodeops import probe as P

pytestmark = pytest.mark.gpu


class Stage:
    def __init__(self, run, load, entry, make_opts, record, result, mirror, rc, small, flip):
        self.run = run              # run_*_records
        self.load = load            # the library
        self.entry = entry          # its *_records entry
        self.make_opts = make_opts  # keywords -> the C options
        self.record = record
        self.result = result
        self.mirror = mirror        # numpy mirror of the stage's aggregate
        self.rc = rc                # of a mismatch
        self.small = small          # options of the smallest run, besides grid and rounds
        self.flip = flip            # self-test mode 1: one expected bit, every wave flags it


STAGES = {
    "compute": Stage(P.run_compute_records, P.load_library, "cro_probe_compute_records",
                     P._compute_opts, P.CroCoverageRecord, P.CroComputeResult,
                     P.aggregate_records, -30, dict(iters=1, lds_bytes=1024),
                     dict(selftest_test="mfma_i8", selftest_elem=13 * 16 + 2, selftest_bit=31)),
    "formats": Stage(F.run_formats_records, F.load_formats_library, "cro_formats_run_records",
                     F._formats_opts, F.CroFormatsRecord, F.CroFormatsResult,
                     F.aggregate_formats_records, F.RC_MISMATCH, dict(iters=1),
                     dict(selftest_test="mx_fp6", selftest_elem=17, selftest_bit=3)),
    "movement": Stage(M.run_movement_records, M.load_movement_library,
                      "cro_movement_run_records", M._movement_opts, M.CroMovementRecord,
                      M.CroMovementResult, M.aggregate_movement_records, M.RC_MISMATCH,
                      dict(iters=1),
                      dict(selftest_test="lds_tr8", selftest_elem=M.movement_elem(1, 1, 63),
                           selftest_bit=9)),
}


@pytest.fixture(params=list(STAGES))
def stage(request):
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU (KFD) on this host")
    return STAGES[request.param]


def test_eight_workgroups_use_every_round_and_each_round_its_own_records(stage):
    """Eight workgroups cannot cover the device, so the run takes all the
    rounds it is allowed; the records come back round-major: round, then
    workgroup, then the workgroup's four waves, which share a CU."""
    res, records = stage.run(0, grid_blocks=8, max_rounds=3, **stage.small)
    assert res["ok"] is True and res["rc"] == 0 and res["msg"] == "ok", res
    assert res["rounds"] == 3 and res["grid_blocks"] == 8, res
    assert records.size == 3 * 8 * 4 and np.all(records["valid"] == 1)
    assert res["waves_run"] == 96 and res["waves_bad"] == 0, res
    assert res["first_bad_round"] == -1 and res["first_bad_record"] == -1, res
    keys = P.cu_key(records["xcc_id"].astype(np.int64),
                    records["hw_id"].astype(np.int64)).reshape(3, 8, 4)
    assert np.all(keys == keys[:, :, :1])
    agg = stage.mirror(records)
    assert agg == {k: res[k] for k in agg}, (agg, res)


def _raw_run(stage, max_records, **opts):
    """The stage's *_records entry on a buffer of eight records of 0xFF bytes:
    the result and the buffer as 8 x 8 words."""
    lib = stage.load(required=True)
    c_opts = stage.make_opts(**opts)
    res = stage.result()
    buf = (stage.record * 8)()
    ctypes.memset(buf, 0xFF, ctypes.sizeof(buf))
    rc = getattr(lib, stage.entry)(0, ctypes.byref(c_opts), ctypes.byref(res), buf, max_records)
    assert ctypes.sizeof(buf) == 8 * 32
    return P._result_dict(res, rc), np.frombuffer(buf, dtype=np.uint32).reshape(8, 8).copy()


@pytest.mark.parametrize("max_records", [5, 0])
def test_no_more_than_max_records_are_copied_out(stage, max_records):
    """Two workgroups report eight waves; the caller's buffer takes the first
    max_records of them and keeps its bytes after that."""
    res, words = _raw_run(stage, max_records, grid_blocks=2, max_rounds=1, **stage.small)
    assert res["ok"] is True and res["rc"] == 0 and res["waves_run"] == 8, res
    assert res["rounds"] == 1 and res["waves_bad"] == 0, res
    assert np.all(words[max_records:] == 0xFFFFFFFF)
    names = [name for name, _ in stage.record._fields_]
    got = {name: words[:max_records, i] for i, name in enumerate(names)}
    assert np.all(got["valid"] == 1) and np.all(got["reserved"] == 0)
    assert np.all(got["fail_mask"] == 0) and np.all(got["n_bad"] == 0)
    assert np.all(got["first_bad"] == 0xFFFFFFFF) and np.all(got["bits_bad"] == 0)
    # the four waves of a workgroup share a CU
    keys = P.cu_key(got["xcc_id"].astype(np.int64), got["hw_id"].astype(np.int64))
    assert np.all(keys[:4] == keys[:1])


def _place(res):
    return "xcd=%d se=%d sh=%d cu=%d simd=%d" % tuple(
        res[k] for k in ("xcd", "se", "sh", "cu", "simd"))


def test_a_mismatch_ends_the_run_whatever_rounds_are_left(stage):
    """Every wave of round 1 is bad: with three rounds allowed the run stops
    after the first as it does with one, and reports the same."""
    flip = dict(grid_blocks=2, selftest_mode=1, **stage.small, **stage.flip)
    one, one_records = stage.run(0, max_rounds=1, **flip)
    res, records = stage.run(0, max_rounds=3, **flip)
    for r, rec in ((one, one_records), (res, records)):
        assert r["ok"] is False and r["rc"] == stage.rc, r
        assert r["rounds"] == 1 and rec.size == 8 and r["waves_bad"] == r["waves_run"] == 8, r
        assert r["first_bad_round"] == 0 and r["first_bad_record"] == 0, r
        assert r["failed_test"] == stage.flip["selftest_test"] and _place(r) in r["msg"], r
    assert (res["rc"], res["failed_test"]) == (one["rc"], one["failed_test"])
    # the message names where the first bad wave ran, which is each run's own
    # (wave 0 of workgroup 0 is placed by the hardware); all else is the same
    assert res["msg"] == one["msg"].replace(_place(one), _place(res))
