"""GPU-marked tests of the coherence probe stage on a real MI355X.

Every comparison is bit-exact: the tally lines as downloaded against the numpy
mirror of crocoherence.h, the pair counts of the visibility check against
n(n-1)/2.  Detection and localisation are shown with the stage's self-test
modes, which alter one bit of an expected value (mode 1), make the workgroup on
one CU misbehave with data only (mode 2) or leave the consumer's acquire fence
out (mode 3, which only reads old data): nothing on the GPU is provoked, and no
kernel of the stage ever waits for another workgroup.
"""

import os

import numpy as np
import pytest

from cro_amd.nodeops import coherence as C
from cro_amd.nodeops import probe as probe_mod

pytestmark = pytest.mark.gpu


def _require_gpu():
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU (KFD) on this host")


_cache = {}


def _clean():
    """One clean run at the default grid with two epochs, its records and
    its tally units, shared and read-only."""
    if "clean" not in _cache:
        res, records, units = C.run_coherence_records(0, iters=2)
        records.setflags(write=False)
        units.setflags(write=False)
        _cache["clean"] = (res, records, units)
    return _cache["clean"]


def _pairs(grid):
    return sum(min(64, grid - g0) * (min(64, grid - g0) - 1) // 2 for g0 in range(0, grid, 64))


def _key(records, block):
    """CU key of the CU a block of the clean run's first epoch ran on."""
    return ((int(records["xcc_id"][block * 4]) & 0xF) << 16) | (
        int(records["hw_id"][block * 4]) & 0xFF00)


def _blocks_on(records, grid, key):
    keys = ((records["xcc_id"].astype(np.int64) & 0xF) << 16) | (
        records["hw_id"].astype(np.int64) & 0xFF00)
    return sorted(set(records["block"][keys == key].tolist()))


def test_clean_run_covers_every_cu_and_every_tally_is_exact():
    _require_gpu()
    res, records, units = _clean()
    assert res["ok"] and res["rc"] == 0 and res["failed_test"] == "", res
    grid = res["grid_blocks"]
    assert grid == res["cus_expected"] and res["cus_seen"] == res["cus_expected"]
    assert res["xcds_seen"] == 8 and res["simds_seen"] == 4 * res["cus_seen"]
    assert res["iters"] == 2 and res["waves_run"] == res["rounds"] * 2 * grid * 4
    assert res["pairs_checked"] == res["pairs_expected"] == res["rounds"] * 2 * _pairs(grid)
    assert res["vis_bad"] == 0 and res["vis_stale"] == 0 and res["fail_mask"] == 0
    assert units.shape == (2, C.coherence_units(grid), C.UNIT_WORDS)
    per = grid * 4
    for e in range(2):
        launch = records[e * per:(e + 1) * per]
        assert (launch["valid"] == 1).all() and (launch["epoch"] == e + 1).all()
        assert (launch["fail_mask"] == 0).all()
        xcc = launch["xcc_id"].reshape(grid, 4)
        assert (xcc == xcc[:, :1]).all()  # a workgroup's waves share its XCD
        want = C.expected_units(grid, 0, e + 1, xcc[:, 0])
        assert np.array_equal(units[e], want), np.argwhere(units[e] != want)[:8]
    # the mirror's aggregate of the same records
    agg = C.aggregate_coherence_records(records, grid, 2)
    assert agg["pairs_checked"] == 2 * _pairs(grid) and agg["cus_seen"] == res["cus_seen"]
    assert agg["fail_mask"] == 0


@pytest.mark.parametrize("grid,pairs", [(1, 0), (2, 1), (65, 64 * 63 // 2)])
def test_the_smallest_grids_that_can_still_go_wrong(grid, pairs):
    _require_gpu()
    res, records, units = C.run_coherence_records(0, grid_blocks=grid, iters=2, max_rounds=1)
    assert res["ok"] and res["grid_blocks"] == grid and res["rounds"] == 1, res
    assert res["pairs_checked"] == res["pairs_expected"] == 2 * pairs
    for e in range(2):
        launch = records[e * grid * 4:(e + 1) * grid * 4]
        want = C.expected_units(grid, 0, e + 1, launch["xcc_id"][::4])
        assert np.array_equal(units[e], want)
        if grid == 1:
            # one workgroup: its XCD line holds what the wide rules give that
            # workgroup alone, and the shared slots equal the workgroup line's
            xcd_line = units[e][C.xcd_unit(1, int(launch["xcc_id"][0]), 0)]
            shared = [0, 1, 2, 3] + list(range(6, 18))
            assert np.array_equal(xcd_line[shared], units[e][0][shared])
            assert np.array_equal(xcd_line, units[e][C.dev_unit(1, 0)])
        if grid == 65:
            # two arrival words: the second has one block and no pair
            assert int(launch["vis_pairs"][64 * 4:].sum()) == 0
            assert int(launch["vis_pairs"][:64 * 4].sum()) == pairs


@pytest.mark.parametrize("test", C.COHERENCE_TESTS)
def test_mode_1_a_flipped_expected_value_fails_with_that_check(test):
    _require_gpu()
    res = C.run_coherence(0, iters=2, selftest_mode=1, selftest_test=test, selftest_bit=3)
    assert res["rc"] == C.RC_MISMATCH and res["ok"] is False, res
    assert res["failed_test"] == test and test in res["msg"]
    assert res[f"bad_{test}"] >= 1
    others = [t for t in C.COHERENCE_TESTS if t != test and res[f"bad_{t}"]]
    assert others == [], others


def test_mode_2_a_dropped_add_names_the_cu_and_its_lines():
    _require_gpu()
    clean, records, _ = _clean()
    grid = clean["grid_blocks"]
    key = _key(records, 41)
    res, rec, units = C.run_coherence_records(0, iters=1, max_rounds=1, selftest_mode=2,
                                              selftest_test="add_u32", selftest_key=key)
    assert res["rc"] == C.RC_MISMATCH and res["failed_test"] == "add_u32", res
    # the workgroups that ran on that CU in this launch (one, as a rule)
    victims = _blocks_on(rec, grid, key)
    assert victims and res["bad_block"] == victims[0]
    loc = probe_mod.decode_cu_key(key)
    assert res["tally_level"] == 0 and res["tally_unit"] == victims[0]
    assert (res["xcd"], res["se"], res["sh"], res["cu"]) == (
        loc["xcd"], loc["se"], loc["sh"], loc["cu"])
    # their workgroup lines, XCD lines and device lines are short by the
    # dropped lanes' own amounts, and nothing else differs
    xcc = rec["xcc_id"][::4]
    full = C.expected_units(grid, 0, 1, xcc)
    short = C.expected_units(grid, 0, 1, xcc, drop=(victims, "add_u32"))
    assert np.array_equal(units[0], short)
    lines = sorted({int(u) for u in np.argwhere(units[0] != full)[:, 0]})
    want_lines = set()
    for b in victims:
        want_lines |= {b, C.xcd_unit(grid, int(xcc[b]), b), C.dev_unit(grid, b)}
    assert lines == sorted(want_lines)
    salt = C.coherence_salt(0, 1)
    for b in victims:
        amount = int(C.lane_values(b, salt, 0)["add_u32"][0])
        assert (int(full[b, 0]) - int(units[0][b, 0])) & 0xFFFFFFFF == amount
    assert res["bad_add_u32"] == len(lines) and res["waves_bad"] == 0
    assert [t for t in C.COHERENCE_TESTS if t != "add_u32" and res[f"bad_{t}"]] == []


@pytest.mark.parametrize("test", ["ticket", "lds_rmw", "visibility"])
def test_mode_2_names_exactly_the_expected_party(test):
    _require_gpu()
    clean, records, _ = _clean()
    grid = clean["grid_blocks"]
    key = _key(records, 9)
    res, rec, _ = C.run_coherence_records(0, iters=2, max_rounds=1, selftest_mode=2,
                                          selftest_test=test, selftest_bit=7, selftest_key=key)
    assert res["rc"] == C.RC_MISMATCH and res["failed_test"] == test, res
    per = grid * 4
    launches = [rec[e * per:(e + 1) * per] for e in range(2)]
    victims = [_blocks_on(launch, grid, key) for launch in launches]
    assert victims[0] or victims[1]
    loc = probe_mod.decode_cu_key(key)
    place = tuple(loc[k] for k in ("xcd", "se", "sh", "cu"))
    assert res["bad_block"] in victims[0] + victims[1]
    assert [t for t in C.COHERENCE_TESTS if t != test and res[f"bad_{t}"]] == []
    if test == "ticket":
        # one ticket per such workgroup left unmarked, drawn by its lane 0
        assert res["bad_ticket"] == len(victims[0]) + len(victims[1]) and res["ticket_seen"] == 0
        assert res["ticket_owner"] == res["bad_block"] * 256 and res["waves_bad"] == 0
        assert (res["xcd"], res["se"], res["sh"], res["cu"]) == place
    elif test == "lds_rmw":
        for launch, blocks in zip(launches, victims):
            bad = launch[launch["fail_mask"] != 0]
            assert bad["block"].tolist() == blocks  # wave 0 of each, nobody else
            assert (bad["fail_mask"] == 1 << 10).all() and (bad["first_bad"] == 0).all()
            assert (bad["bits_bad"] == 1 << 7).all() and (bad["n_bad"] == 1).all()
        assert res["cus_bad"] == 1
        assert (res["xcd"], res["se"], res["sh"], res["cu"]) == place
    else:
        # every consumer that saw such a producer's bit reports that block,
        # dword 5, one bit, not stale; nobody reports anything else
        n_bad = 0
        for launch, blocks in zip(launches, victims):
            bad = launch[launch["fail_mask"] != 0]
            n_bad += len(bad)
            assert (bad["fail_mask"] == 1 << 11).all()
            assert set(bad["vis_first_block"].tolist()) <= set(blocks)
            assert (bad["vis_first_dword"] == 5).all() and (bad["vis_bits"] == 1 << 7).all()
            assert not set(bad["block"].tolist()) & set(blocks) or len(blocks) > 1
            for b in blocks:
                group = set(range(b & ~63, min(grid, (b & ~63) + 64)))
                seen_by = set(bad["block"][bad["vis_first_block"] == b].tolist())
                assert seen_by <= group - {b}
        assert n_bad >= 1 and res["vis_stale"] == 0 and res["vis_bad"] >= n_bad
        assert res["pairs_checked"] == res["pairs_expected"]


def test_mode_3_without_the_acquire_only_stale_values_appear():
    _require_gpu()
    res = C.run_coherence(0, iters=2, max_rounds=1, selftest_mode=3)
    for name in C.COHERENCE_TESTS[:C.TALLY_TESTS]:
        assert res[f"bad_{name}"] == 0, res
    assert res["vis_bad"] == res["vis_stale"], res


def test_the_coverage_floor():
    _require_gpu()
    res = C.run_coherence(0, grid_blocks=8, max_rounds=1, min_cu_fraction=1.0)
    assert res["rc"] == C.RC_COVERAGE and res["ok"] is False, res
    assert res["cus_seen"] <= 8 and res["fail_mask"] == 0 and "coverage" in res["msg"]


def test_through_the_probe_hook_on_the_real_device():
    _require_gpu()

    class Gpu:
        pci_bdf = "0000:00:00.0"  # unknown: the hook falls back to ordinal 0

    fn = probe_mod.make_probe_fn("quick", coherence=True)
    result = fn(Gpu())
    assert result["ok"] is True, result
    assert result["coherence"]["ok"] is True
    assert result["coherence"]["cus_seen"] == result["coherence"]["cus_expected"]
