"""GPU-marked tests of the data-movement probe stage on a real MI355X.

Every comparison is bit-exact: what one wave of the stage's own device
functions delivers through the tile entry against the numpy mirrors of
cromovement.h, one-hot sweeps of the transposed reads and of LDS-DMA, and the
stage itself.  Detection and localisation are shown with the stage's self-test
modes, which flip one bit of an expected word (mode 1) or of a received word
on one CU (mode 2): data only, nothing on the GPU is provoked.
"""

import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from cro_amd.nodeops import movement as M
from cro_amd.nodeops import probe as probe_mod

pytestmark = pytest.mark.gpu

AGENT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                     "cro_amd", "agent", "croagent")
REGISTER_CHECKS = (M.DPP, M.SWIZZLE, M.BPERMUTE, M.PLSWAP, M.READLANE)
TR_CHECKS = (M.TR16, M.TR8, M.TR4, M.TR6)
ALL_VARIANTS = [(t, v) for t in range(len(M.MOVEMENT_TESTS)) for v in range(M.movement_variants(t))]


def _require_gpu():
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU (KFD) on this host")


_cache = {}


def _clean():
    """One clean run at the library defaults and its records, shared and
    read-only."""
    if "clean" not in _cache:
        res, records = M.run_movement_records(0)
        records.setflags(write=False)
        _cache["clean"] = (res, records)
    return _cache["clean"]


def _distinct_words(seed):
    rng = np.random.default_rng(seed)
    return (rng.permutation(1 << 24)[:128] + 1).astype(np.uint32).reshape(2, 64)


# -- tile entry: the maps ----------------------------------------------------------------------


@pytest.mark.parametrize("seed", (0, 5))
@pytest.mark.parametrize("t,v", [tv for tv in ALL_VARIANTS if tv[0] in REGISTER_CHECKS])
def test_tile_register_checks_equal_the_mirror(t, v, seed):
    _require_gpu()
    data = _distinct_words(seed)
    rt = M.movement_rt(seed, 3)
    addr = None
    if t == M.BPERMUTE:
        addr = M.bperm_index(v, rt)
    elif t == M.READLANE:
        addr = np.zeros(64, dtype=np.int32)
        addr[0] = (rt["sel"], 0, rt["fa"], rt["wl"])[v]
    want = M.apply_source_map(M.movement_source_map(t, v, rt), data)
    got = M.movement_tile(0, t, v, data, addr)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    # neither the identity nor the mirror image of the input passes for it
    assert not np.array_equal(want[0], data[0])
    assert not np.array_equal(want[0], data[0][::-1])
    if t == M.BPERMUTE and v != 2:
        assert np.array_equal(got[0], M.bperm_apply(v, addr, data[0]))


def test_tile_swizzle_reverse_works_per_32_lanes():
    _require_gpu()
    data = _distinct_words(1)
    got = M.movement_tile(0, M.SWIZZLE, 2, data)[0]
    assert np.array_equal(got[:32], data[0][:32][::-1])
    assert np.array_equal(got[32:], data[0][32:][::-1])
    assert not np.array_equal(got, data[0][::-1])  # not a reverse of the whole wave


@pytest.mark.parametrize("seed", (0, 5))
@pytest.mark.parametrize("t,v", [tv for tv in ALL_VARIANTS if tv[0] in TR_CHECKS])
def test_tile_transposed_reads_equal_the_mirror(t, v, seed):
    _require_gpu()
    salt = M.movement_salt(seed, 3)
    image, addr = M.tr_image(t, v, salt), M.tr_addr(t, v)
    got = M.movement_tile(0, t, v, image.view(np.uint8), addr)
    want = M.tr_want(t, v, salt)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(want, M.tr_read(t, image, addr))
    # an untransposed read of the same addresses would have given this
    plain = np.stack([image.view(np.uint8)[a:a + M.TR_TABLE[t][3]].view(np.uint32)
                      for a in addr]).T
    assert not np.array_equal(want, plain)


@pytest.mark.parametrize("t", TR_CHECKS)
def test_one_hot_sweep_of_a_transposed_read(t):
    """One non-zero element at a time over every element of one block, in the
    first and the last 16-lane group: exactly one destination field receives
    it, and it is the mirror's (for 6-bit fields this walks the fields across
    the dword boundaries)."""
    _require_gpu()
    bits, rows, per, nbytes = M.TR_TABLE[t]
    stride, addr = M.tr_stride(t, 1), M.tr_addr(t, 1)
    ones = (1 << bits) - 1
    row_words = 16 * bits // 32
    for group in (0, 3):
        for row in range(rows):
            for col in range(16):
                elems = np.zeros((4, rows, 16), dtype=np.uint32)
                elems[group, row, col] = ones
                image = np.zeros((4, rows, stride // 4), dtype=np.uint32)
                image[:, :, :row_words] = M._pack(elems, bits, row_words)
                got = M.movement_tile(0, t, 1, image.reshape(-1).view(np.uint8), addr)
                fields = M._unpack(got.T.copy(), bits, rows)  # lane, field
                hits = np.argwhere(fields != 0).tolist()
                assert hits == [[16 * group + col, row]], (group, row, col, hits)
                assert fields[16 * group + col, row] == ones
                assert np.array_equal(got, M.tr_read(t, image.reshape(-1), addr))


@pytest.mark.parametrize("seed", (0, 5))
@pytest.mark.parametrize("v", (0, 1, 2))
def test_tile_dma_equals_the_mirror_and_leaves_the_guard_bands(v, seed):
    _require_gpu()
    src = M.dma_source_words()
    rt = M.movement_rt(seed, 3)
    addr = M.dma_addr(v, 2, rt)
    got = M.movement_tile(0, M.DMA, v, src.view(np.uint8), addr)
    want = M.dma_read(v, src, addr)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    n = M.dma_size(v) // 4
    assert (got[n] == M.POISON).all()
    # not what an identity gather, or one without the instruction offset, gives
    linear = np.arange(64) * M.dma_size(v) + 2048
    assert not np.array_equal(want, M.dma_read(v, src, linear))
    if v == 2:
        assert not np.array_equal(want[:n], M.dma_read(0, src, addr)[:n])


@pytest.mark.parametrize("v", (0, 1, 2))
def test_one_hot_sweep_of_the_dma_source_chunks(v):
    """One non-zero source chunk at a time: its words land in the one lane's
    destination slot the mirror names, everything else stays zero and the
    guard bands stay poisoned."""
    _require_gpu()
    size, n = M.dma_size(v), M.dma_size(v) // 4
    rt = M.movement_rt(5, 1)
    addr = M.dma_addr(v, 0, rt)
    for lane in range(64):
        src = np.zeros(M.SRC_WORDS, dtype=np.uint32)
        first = (int(addr[lane]) + M.dma_ioff(v)) // 4
        src[first:first + n] = 0xC0DE0001 + np.arange(n, dtype=np.uint32)
        got = M.movement_tile(0, M.DMA, v, src.view(np.uint8), addr)
        data = got[:n].reshape(-1)
        hits = np.flatnonzero(data).tolist()
        assert hits == list(range(lane * n, (lane + 1) * n)), (lane, hits)
        assert data[hits].tolist() == src[first:first + n].tolist()
        assert (got[n] == M.POISON).all()
        assert size * 64 == data.size * 4


def test_tile_rejects_what_it_cannot_run_in_bounds():
    _require_gpu()
    data = _distinct_words(0)
    with pytest.raises(RuntimeError, match="rc=-10"):
        M.movement_tile(0, M.BPERMUTE, 0, data, np.full(64, 64))
    with pytest.raises(RuntimeError, match="rc=-10"):
        M.movement_tile(0, M.TR16, 0, np.zeros(512, dtype=np.uint8), np.full(64, 508))
    with pytest.raises(RuntimeError, match="rc=-10"):
        M.movement_tile(0, M.TR8, 0, np.zeros(512, dtype=np.uint8), np.full(64, 4))
    with pytest.raises(RuntimeError, match="rc=-10"):
        M.movement_tile(0, M.DMA, 2, np.zeros(1024, dtype=np.uint8), np.full(64, 960))
    with pytest.raises(RuntimeError, match="rc=-10"):
        M.movement_tile(0, M.READLANE, 2, data, np.zeros(64, dtype=np.int32))


# -- the stage ---------------------------------------------------------------------------------


@pytest.mark.parametrize("seed", (0, 5))
@pytest.mark.parametrize("grid,iters", [(1, 1), (2, 1), (0, 1), (1, 0), (2, 65)])
def test_stage_is_clean(grid, iters, seed):
    _require_gpu()
    res, records = M.run_movement_records(0, grid_blocks=grid, iters=iters, seed=seed)
    assert res["ok"] and res["rc"] == 0 and res["failed_test"] == "" and res["msg"] == "ok", res
    assert res["fail_mask"] == 0 and res["waves_bad"] == 0 and res["first_bad_index"] == -1
    assert res["waves_run"] == res["rounds"] * res["grid_blocks"] * 4 == len(records)
    assert (records["valid"] == 1).all() and (records["fail_mask"] == 0).all()
    assert (records["first_bad"] == 0xFFFFFFFF).all()
    if grid:
        assert res["grid_blocks"] == grid and res["cus_seen"] <= grid * res["rounds"]
    if iters:
        assert res["iters"] == iters
    agg = M.aggregate_movement_records(records)
    assert all(agg[k] == res[k] for k in agg), (agg, res)


def test_default_run_reaches_every_cu_xcd_and_simd():
    _require_gpu()
    res, records = _clean()
    assert res["ok"], res
    assert res["grid_blocks"] == res["cus_expected"]
    assert res["cus_seen"] == res["cus_expected"], res
    assert res["xcds_seen"] == 8 and res["simds_seen"] == 4 * res["cus_seen"]
    assert 1 <= res["rounds"] <= 4 and res["iters"] >= 1 and res["gpu_ms"] > 0
    keys = probe_mod.cu_key(records["xcc_id"].astype(np.int64), records["hw_id"].astype(np.int64))
    assert np.unique(keys).size == res["cus_expected"]


MODE1_ELEMS = {
    # per check: elements in lane 0, lane 63 and the last register
    M.DPP: [(0, 0, 0), (12, 0, 63)],
    M.SWIZZLE: [(0, 0, 0), (4, 0, 63)],
    M.BPERMUTE: [(1, 0, 0), (2, 0, 63)],
    M.PLSWAP: [(0, 0, 0), (1, 1, 63)],
    M.READLANE: [(2, 0, 0), (3, 0, 63)],
    M.TR16: [(0, 0, 0), (1, 1, 63)],
    M.TR8: [(0, 0, 0), (1, 1, 63)],
    M.TR4: [(0, 0, 0), (1, 1, 63)],
    M.TR6: [(0, 0, 0), (1, 2, 63)],
    M.DMA: [(0, 0, 0), (1, 4, 63), (2, 1, 63)],
}


@pytest.mark.parametrize("bit", (0, 31))
@pytest.mark.parametrize("t", range(len(M.MOVEMENT_TESTS)))
def test_mode_1_every_wave_flags_exactly_that_check_and_element(t, bit):
    _require_gpu()
    name = M.MOVEMENT_TESTS[t]
    for v, r, lane in MODE1_ELEMS[t]:
        elem = M.movement_elem(v, r, lane)
        res, records = M.run_movement_records(0, grid_blocks=2, iters=3, max_rounds=1,
                                              selftest_mode=1, selftest_test=name,
                                              selftest_bit=bit, selftest_elem=elem)
        assert res["rc"] == M.RC_MISMATCH and res["ok"] is False, res
        assert res["failed_test"] == name and name in res["msg"]
        assert f"variant {v} register {r} lane {lane}," in res["msg"]
        assert res["fail_mask"] == 1 << t and res["waves_bad"] == res["waves_run"] == 8
        assert res[f"bad_{name}"] == 8
        assert (records["fail_mask"] == 1 << t).all() and (records["first_bad"] == elem).all()
        assert (records["bits_bad"] == 1 << bit).all()
        # one element, compared once per repeat
        assert (records["n_bad"] == 3).all() and res["n_bad"] == 3
        assert res["first_bad"] == elem and res["bits_bad"] == 1 << bit
        assert res["first_bad_round"] == 0 and res["first_bad_record"] == 0


def test_mode_1_two_checks_at_once_the_lower_leads():
    _require_gpu()
    elem = M.movement_elem(1, 1, 40)
    res, records = M.run_movement_records(0, grid_blocks=1, iters=1, max_rounds=1,
                                          selftest_mode=1, selftest_test="lds_tr4",
                                          selftest_bit=9, selftest_elem=elem,
                                          selftest_also="permlane_swap")
    assert res["rc"] == M.RC_MISMATCH and res["failed_test"] == "permlane_swap", res
    assert res["fail_mask"] == (1 << M.TR4) | (1 << M.PLSWAP)
    assert (records["fail_mask"] == res["fail_mask"]).all()
    assert res["bad_permlane_swap"] == res["bad_lds_tr4"] == 4
    assert res["first_bad"] == elem and res["n_bad"] == 1


def test_mode_2_exactly_the_waves_of_that_cu_are_flagged():
    _require_gpu()
    clean, clean_records = _clean()
    key = int(probe_mod.cu_key(int(clean_records["xcc_id"][41 * 4]),
                               int(clean_records["hw_id"][41 * 4])))
    elem = M.movement_elem(1, 0, 33)
    res, records = M.run_movement_records(0, iters=1, selftest_mode=2, selftest_test="lds_dma",
                                          selftest_bit=17, selftest_elem=elem, selftest_key=key)
    assert res["rc"] == M.RC_MISMATCH and res["failed_test"] == "lds_dma", res
    keys = probe_mod.cu_key(records["xcc_id"].astype(np.int64), records["hw_id"].astype(np.int64))
    on_cu = keys == key
    assert on_cu.any()
    assert ((records["fail_mask"] != 0) == on_cu).all()
    bad = records[on_cu]
    assert (bad["fail_mask"] == 1 << M.DMA).all() and (bad["first_bad"] == elem).all()
    assert (bad["bits_bad"] == 1 << 17).all() and (bad["n_bad"] == 1).all()
    loc = probe_mod.decode_cu_key(key)
    assert (res["xcd"], res["se"], res["sh"], res["cu"]) == tuple(
        loc[k] for k in ("xcd", "se", "sh", "cu"))
    assert res["cus_bad"] == 1 and res["waves_bad"] == int(on_cu.sum())


def test_the_coverage_floor_and_bad_arguments():
    _require_gpu()
    res = M.run_movement(0, grid_blocks=8, max_rounds=1, min_cu_fraction=1.5)
    assert res["rc"] == M.RC_COVERAGE and res["ok"] is False, res
    assert res["fail_mask"] == 0 and res["waves_bad"] == 0 and "coverage" in res["msg"]
    for bad in (dict(grid_blocks=-1), dict(iters=-1), dict(max_rounds=65),
                dict(min_cu_fraction=-0.5), dict(selftest_mode=3),
                dict(selftest_mode=1, selftest_test="dpp", selftest_elem=M.movement_elem(13, 0, 0)),
                dict(selftest_mode=1, selftest_test="lds_tr6", selftest_elem=M.movement_elem(0, 3, 0)),
                dict(selftest_mode=1, selftest_test="dpp", selftest_bit=32),
                dict(selftest_mode=1, selftest_test="lds_tr6", selftest_also="dpp",
                     selftest_elem=M.movement_elem(0, 2, 0)),
                dict(selftest_also="dpp")):
        res = M.run_movement(0, **bad)
        assert res["rc"] == -1 and res["ok"] is False and "bad argument" in res["msg"], (bad, res)
    assert M.run_movement(99)["rc"] == -1


def test_four_threads_on_one_device_agree():
    _require_gpu()
    with ThreadPoolExecutor(max_workers=4) as pool:
        results = list(pool.map(lambda seed: M.run_movement(0, grid_blocks=4, iters=2, seed=seed),
                                (0, 5, 0, 5)))
    drop = ("gpu_ms", "t_total_ms", "rounds", "waves_run", "cus_seen", "xcds_seen", "simds_seen")
    assert all(r["ok"] for r in results), results
    same = [{k: v for k, v in r.items() if k not in drop} for r in results]
    assert same[0] == same[1] == same[2] == same[3]


def test_croagent_probe_movement_prints_what_python_reports():
    _require_gpu()
    run = subprocess.run([AGENT, "probe", "--device", "0", "--movement"], capture_output=True,
                         text=True, timeout=120)
    out = json.loads(run.stdout)
    assert run.returncode == 0 and out["ok"] is True, run.stdout
    mine = M.run_movement(0)
    theirs = out["movement"]
    assert list(theirs) == list(mine)
    timing = ("gpu_ms", "t_total_ms")
    if theirs["rounds"] != mine["rounds"]:  # placement may take another round
        timing += ("rounds", "waves_run")
    assert {k: v for k, v in theirs.items() if k not in timing} == {
        k: v for k, v in mine.items() if k not in timing}
    floor = subprocess.run([AGENT, "probe", "--device", "0", "--movement",
                            "--movement-min-cu-fraction", "1.5"], capture_output=True, text=True,
                           timeout=120)
    out = json.loads(floor.stdout)
    assert floor.returncode == 1 and out["ok"] is False and out["movement"]["rc"] == M.RC_COVERAGE
    assert out["msg"] == out["movement"]["msg"]


def test_through_the_probe_hook_on_the_real_device():
    _require_gpu()

    class Gpu:
        pci_bdf = "0000:00:00.0"  # unknown: the hook falls back to ordinal 0

    fn = probe_mod.make_probe_fn("quick", movement=True)
    result = fn(Gpu())
    assert result["ok"] is True, result
    assert result["movement"]["ok"] is True
    assert result["movement"]["cus_seen"] == result["movement"]["cus_expected"]
