"""GPU-marked tests of the ALU probe stage on a real MI355X.

Every comparison is bit-exact: what one wave of the stage's own device code
delivers through the tile entry, form by form, against the Python reference of
nodeops/alu.py (on the stage's own rows for two seeds and on caller rows), the
transcendental anchors, and the stage itself.  Detection and localisation are
shown with the stage's self-test modes, which flip one bit of an expected word
(mode 1) or of a computed word on one CU (mode 2): data only, nothing on the
GPU is provoked.
"""

import json
import os
import subprocess

import numpy as np
import pytest

from cro_amd.nodeops import alu as A
from cro_amd.nodeops import probe as probe_mod

pytestmark = pytest.mark.gpu

AGENT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                     "cro_amd", "agent", "croagent")
CHECKS = range(len(A.ALU_TESTS))
# one form of every check for the self-tests: (form, word)
SELFTEST_FORMS = ("mad_u64_u32", "perm_b32", "pk_mad_i16", "dot4_i32_i8", "fma_f32", "pk_fma_f16",
                  "fma_f64", "cvt_pk_bf16_f32", "sc_pk_fp8_f32", "cmp_lt_f32", "s_mul_hi_u32",
                  "t_rcp_f32")


def _require_gpu():
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU (KFD) on this host")


_cache = {}


def _table(seed):
    if ("table", seed) not in _cache:
        table = A.alu_table(seed)
        table.setflags(write=False)
        _cache["table", seed] = table
    return _cache["table", seed]


def _clean():
    """One clean run at the library defaults and its records, shared and read-only."""
    if "clean" not in _cache:
        res, records = A.run_alu_records(0)
        records.setflags(write=False)
        _cache["clean"] = (res, records)
    return _cache["clean"]


def _forms_of_check(check):
    return [f for f, fm in enumerate(A.alu_forms()) if fm[0] == check]


# -- tile entry: every reference -------------------------------------------------------------


@pytest.mark.parametrize("seed", (0, 5))
@pytest.mark.parametrize("check", CHECKS, ids=A.ALU_TESTS)
def test_tile_every_form_equals_the_reference_on_the_stages_rows(check, seed):
    _require_gpu()
    table = _table(seed)
    for f in _forms_of_check(check):
        name, sig = A.alu_forms()[f][1], A.alu_forms()[f][3]
        got = A.alu_tile(0, f, table[f, :, :6])
        rows, nres = A.checked_rows(f), A.SIGS[sig][1]
        want = table[f, :rows, 6:6 + nres]
        assert np.array_equal(got[:rows, :nres], want), (name, np.argwhere(got[:rows, :nres] != want)[:4])
        if nres == 1:
            assert not got[:, 1].any()


def test_tile_integer_forms_equal_the_reference_on_caller_rows():
    _require_gpu()
    rng = np.random.default_rng(7)
    rows = rng.integers(0, 1 << 32, size=(64, 6), dtype=np.uint64).astype(np.uint32)
    rows[:, 1] &= np.where(np.arange(64) % 2 == 0, 0xFFFFFFFF, 63).astype(np.uint32)
    forms = [f for f, fm in enumerate(A.alu_forms()) if fm[4] == "INT"]
    assert len(forms) > 100
    for f in forms:
        want = np.array([A.alu_reference(f, r) for r in rows], dtype=np.uint32)
        if A.alu_forms()[f][3] == "V1_MBCNT":  # the one result that depends on the lane
            want[:, 0] = [A.alu_mbcnt(int(r[0]), int(r[1]), int(r[2]), lane)
                          for lane, r in enumerate(rows)]
        got = A.alu_tile(0, f, rows)
        assert np.array_equal(got, want), A.alu_forms()[f][1]


def test_tile_old_payload_is_kept_where_the_form_says_so():
    _require_gpu()
    # UNUSED_PRESERVE, op_sel word select and the masked v_mov under v_cmpx:
    # what was kept and what was written differ in every row
    table = _table(0)
    for name, old_word, keep_mask in (("ashr_pk_i8_i32", 3, 0xFFFF0000), ("sc_pk_fp8_f16", 2, 0xFFFF0000),
                                      ("add_u32_sdwa", 2, 0x0000FFFF), ("sub_u32_sdwa", 2, 0xFFFF00FF),
                                      ("fma_f16", 3, 0xFFFF0000), ("fma_mixlo_f16", 3, 0xFFFF0000), ("fma_mixhi_f16", 3, 0x0000FFFF),
                                      ("sc_pk_fp8_f32", 3, 0xFFFF0000), ("sc_pk_fp8_f32_hi", 3, 0x0000FFFF)):
        f = A.form_index(name)
        got = A.alu_tile(0, f, table[f, :, :6])[:, 0]
        old = table[f, :, old_word]
        assert np.array_equal(got & keep_mask, old & keep_mask), name
        assert np.any((got & ~np.uint32(keep_mask)) != (old & ~np.uint32(keep_mask))), name
    f = A.form_index("cmpx_lt_u32")
    got, rows = A.alu_tile(0, f, table[f, :, :6])[:, 0], table[f]
    less = rows[:, 0] < rows[:, 1]
    assert less.any() and (~less).any()
    assert np.array_equal(got, np.where(less, rows[:, 0], rows[:, 2]))


def test_transcendental_anchors_are_exact():
    _require_gpu()
    # exp of small integers, log and rcp of powers of two, sqrt and rsq of even
    # powers, sin and cos at the quarter revolutions: exact on a healthy device
    for seed in (0, 5):
        table = _table(seed)
        for f in _forms_of_check(A.TRANS):
            name, nres = A.alu_forms()[f][1], A.SIGS[A.alu_forms()[f][3]][1]
            n = A.checked_rows(f)
            assert n == (0 if name == "t_sqrt_f64" else A.ANCHORS)
            got = A.alu_tile(0, f, table[f, :, :6])
            assert np.array_equal(got[:n, :nres], table[f, :n, 6:6 + nres]), name


def test_tile_bad_arguments():
    _require_gpu()
    lib = A.load_alu_library(required=True)
    rows = np.zeros((64, 6), dtype=np.uint32)
    out = np.zeros((64, 2), dtype=np.uint32)
    n = len(A.alu_forms())
    for form, n_in, n_out in ((-1, rows.nbytes, out.nbytes), (n, rows.nbytes, out.nbytes),
                              (0, rows.nbytes - 4, out.nbytes), (0, rows.nbytes, out.nbytes + 4)):
        assert lib.cro_alu_tile(0, form, rows.ctypes.data, n_in, out.ctypes.data, n_out) == -10
    assert lib.cro_alu_tile(0, 0, None, rows.nbytes, out.ctypes.data, out.nbytes) == -10


# -- the stage ------------------------------------------------------------------------------------


def test_clean_run_covers_the_device_and_agrees_on_one_digest():
    _require_gpu()
    res, records = _clean()
    assert res["ok"] and res["rc"] == 0 and res["msg"] == "ok", res
    assert res["cus_seen"] == res["cus_expected"] and res["simds_seen"] == 4 * res["cus_seen"]
    assert res["waves_bad"] == 0 and res["first_bad"] == 0xFFFFFFFF and res["failed_test"] == ""
    assert res["digest_waves"] == res["waves_run"] and res["no_majority"] == 0
    assert len(set(records["digest"].tolist())) == 1 and res["digest"] == int(records["digest"][0])
    mirror = A.aggregate_alu_records(records)
    assert {k: res[k] for k in mirror} == mirror


def test_the_seed_changes_the_table_and_the_digest():
    _require_gpu()
    a, b, c = A.run_alu(0, seed=5), A.run_alu(0, seed=0), A.run_alu(0, seed=5)
    assert a["ok"] and b["ok"] and c["ok"], (a["msg"], b["msg"], c["msg"])
    assert a["digest"] == c["digest"] != b["digest"]
    assert b["digest"] == _clean()[0]["digest"]


def test_sixty_four_repeats_show_every_row_to_every_lane():
    _require_gpu()
    res = A.run_alu(0, iters=64, grid_blocks=8, max_rounds=1)
    assert res["ok"] and res["iters"] == 64 and res["waves_run"] == 32, res


def _elem(name, lane=5, word=0, repeat=0):
    f = A.form_index(name)
    row = repeat if A.is_scalar(f) else (lane + repeat) & 63
    return f, A.alu_elem(f, word, row, lane)


@pytest.mark.parametrize("check", CHECKS, ids=A.ALU_TESTS)
def test_selftest_expected_word_flip_is_found_and_located(check):
    _require_gpu()
    name = SELFTEST_FORMS[check]
    f, elem = _elem(name)
    assert A.alu_forms()[f][0] == check
    res = A.run_alu(0, selftest_mode=1, selftest_test=check, selftest_elem=elem, selftest_bit=9)
    assert res["rc"] == A.RC_MISMATCH and not res["ok"], res
    assert res["failed_test"] == A.ALU_TESTS[check] and res["first_fail_mask"] == 1 << check
    assert res["first_bad"] == elem and res["bits_bad"] == 1 << 9
    assert res["waves_bad"] == res["waves_run"] and res[f"bad_{A.ALU_TESTS[check]}"] == res["waves_run"]
    # a scalar form's word is the same in all 64 lanes: one lane is named, one is flipped
    assert res["n_bad"] == 1
    assert f"form {name} word 0" in res["msg"]
    assert A.describe_first_bad(res["first_bad"]).startswith(f"form {A.alu_forms()[f][2]} row")


def test_selftest_the_lowest_failing_check_leads():
    _require_gpu()
    _, elem = _elem("s_mul_hi_u32", lane=0)
    res = A.run_alu(0, selftest_mode=1, selftest_test="salu", selftest_elem=elem, selftest_bit=3,
                    selftest_also="mul_hi_u32")
    assert res["rc"] == A.RC_MISMATCH and res["failed_test"] == "int_arith", res
    assert res["first_fail_mask"] == (1 << A.INT) | (1 << A.SALU)
    assert res["first_bad"] >> 13 == A.form_index("mul_hi_u32")
    assert res["bad_int_arith"] == res["bad_salu"] == res["waves_run"]


def test_selftest_computed_word_flip_on_one_cu_names_that_cu():
    _require_gpu()
    _, records = _clean()
    pick = records[len(records) // 3]
    key = probe_mod.cu_key(int(pick["xcc_id"]), int(pick["hw_id"]))
    loc = probe_mod.decode_location(int(pick["xcc_id"]), int(pick["hw_id"]))
    _, elem = _elem("fma_f64", lane=33, word=1)
    res, recs = A.run_alu_records(0, selftest_mode=2, selftest_test="f64", selftest_elem=elem,
                                  selftest_bit=20, selftest_key=key)
    assert res["rc"] == A.RC_MISMATCH and res["failed_test"] == "f64", res
    assert res["waves_bad"] == 4 and res["cus_bad"] == 1
    assert (res["xcd"], res["se"], res["cu"]) == (loc["xcd"], loc["se"], loc["cu"])
    assert res["first_bad"] == elem and res["bits_bad"] == 1 << 20
    bad = recs[recs["fail_mask"] != 0]
    assert all(probe_mod.cu_key(int(r["xcc_id"]), int(r["hw_id"])) == key for r in bad)
    assert res["digest_waves"] == res["waves_run"]  # no transcendental word was touched


def test_selftest_a_non_anchor_transcendental_word_changes_the_digest():
    _require_gpu()
    res0, records = _clean()
    pick = records[len(records) // 2]
    key = probe_mod.cu_key(int(pick["xcc_id"]), int(pick["hw_id"]))
    f = A.form_index("t_exp_f32")
    elem = A.alu_elem(f, 0, 40, 40)  # row 40 is no anchor
    res = A.run_alu(0, selftest_mode=2, selftest_test="transcendental", selftest_elem=elem,
                    selftest_bit=1, selftest_key=key)
    assert res["rc"] == A.RC_MISMATCH and res["failed_test"] == "transcendental", res
    assert res["waves_bad"] == 4 and res["cus_bad"] == 1 and res["first_bad"] == 0xFFFFFFFF
    assert res["digest"] == res0["digest"] and res["digest_waves"] == res["waves_run"] - 4
    assert "digest differs from the majority's" in res["msg"]
    # mode 1 reaches anchors only: a non-anchor element is a bad argument
    bad = A.run_alu(0, selftest_mode=1, selftest_test="transcendental", selftest_elem=elem)
    assert bad["rc"] == -1 and "selftest_elem" in bad["msg"]


def test_bad_options_and_the_coverage_floor():
    _require_gpu()
    for opts, what in (({"iters": -1}, "iters"), ({"grid_blocks": 1 << 20}, "grid_blocks"),
                       ({"max_rounds": 1000}, "max_rounds"), ({"min_cu_fraction": 3.0}, "min_cu"),
                       ({"selftest_mode": 3}, "selftest_mode"),
                       ({"selftest_mode": 1, "selftest_test": "f32",
                         "selftest_elem": A.alu_elem(0, 0, 0, 0)}, "selftest_elem"),
                       ({"selftest_mode": 1, "selftest_test": "int_arith",
                         "selftest_elem": A.alu_elem(2, 1, 0, 0)}, "selftest_elem"),
                       ({"selftest_also": 3}, "selftest_also")):
        res = A.run_alu(0, **opts)
        assert res["rc"] == -1 and not res["ok"] and what in res["msg"], (opts, res["msg"])
    res = A.run_alu(0, min_cu_fraction=1.5)
    assert res["rc"] == A.RC_COVERAGE and not res["ok"] and res["waves_bad"] == 0, res
    few = A.run_alu(0, grid_blocks=2, max_rounds=2)
    assert few["ok"] and few["cus_seen"] <= 4 and few["rounds"] == 2


def test_staged_probe_and_agent_carry_the_alu_object():
    _require_gpu()

    class Gpu:
        pci_bdf = "none"

    out = probe_mod.make_probe_fn("quick", alu=True)(Gpu())
    assert out["ok"] and out["alu"]["ok"] and list(out)[-1] == "alu", out.get("msg")
    run = subprocess.run([AGENT, "probe", "--alu", "--alu-min-cu-fraction", "0.5"],
                         capture_output=True, text=True, timeout=120)
    agent = json.loads(run.stdout)
    assert run.returncode == 0 and agent["ok"] and agent["alu"]["ok"], agent
    assert list(agent["alu"]) == list(out["alu"])
    assert agent["alu"]["digest"] == out["alu"]["digest"] == _clean()[0]["digest"]
    plain = json.loads(subprocess.run([AGENT, "probe"], capture_output=True, text=True,
                                      timeout=120).stdout)
    assert "alu" not in plain
