"""GPU-marked tests of the compute-coverage probe stage on a real MI355X.

Every comparison is bit-exact: integer data on the i8 and bf16 matrix pipes,
the fmaf chain on the f32 pipe, the address pattern in LDS.  Detection and
localisation are shown with the stage's self-test modes, which alter one bit
of an expected value (mode 1) or of a computed value on the waves of one CU
(mode 2) — data mismatches only; nothing on the GPU is provoked.

Neither of those modes makes an LDS word wrong, and both alter one element in
one lane.  So the march is also shown on real data: a dump entry returns what
the kernel's fill left in LDS (against cropattern.h's numpy mirror, per block,
seed and pass, with a guard after the marched words), and modes 3 and 4 flip
bits in LDS itself, by another wave, between fill and verify, which the clean
run's verify loop must count and locate.  The per-wave tallies get expected
tiles from the caller with several altered elements, in chosen lanes and
registers, and must report the counts, lowest element and bits that numpy
derives from the two tiles.  Small grids and 1 or 2 iterations throughout.

Shapes: the lane-map tiles use one K step and three (accumulation); the clean
runs cross the grid sizes 1 (four records), 8, one workgroup per CU and 44
more than that (more workgroups than CUs) with LDS sizes of 1024 bytes (64
vectors: fewer than the 256 threads), 4096 + 16 (thread 0 takes a second
trip) and 163840 (a CU's whole LDS).
"""

import json
import os
import subprocess
import sys

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
     {"selftest_mode": 3}, {"selftest_mode": 5}, {"selftest_mode": 1, "selftest_test": 4},
     # modes 3 and 4: the LDS test only, span >= 1 and inside LDS, pass 0..2
     {"selftest_mode": 3, "selftest_test": 2, "selftest_span": 1},
     {"selftest_mode": 4, "selftest_test": 0, "selftest_span": 1},
     {"selftest_mode": 3, "selftest_test": 3, "selftest_span": 0},
     {"selftest_mode": 4, "selftest_test": 3, "selftest_span": 0},
     {"selftest_mode": 3, "selftest_test": 3, "selftest_span": 257, "lds_bytes": 1024},
     {"selftest_mode": 3, "selftest_test": 3, "selftest_elem": 255, "selftest_span": 2,
      "lds_bytes": 1024},
     {"selftest_mode": 3, "selftest_test": 3, "selftest_elem": 256, "selftest_span": 1,
      "lds_bytes": 1024},
     {"selftest_mode": 3, "selftest_test": 3, "selftest_elem": 1, "selftest_span": 0xFFFFFFFF,
      "lds_bytes": 1024},
     {"selftest_mode": 4, "selftest_test": 3, "selftest_elem": 40959, "selftest_span": 2},
     {"selftest_mode": 3, "selftest_test": 3, "selftest_span": 1, "selftest_pass": 3},
     {"selftest_mode": 4, "selftest_test": 3, "selftest_span": 1, "selftest_pass": -1},
     {"selftest_mode": 3, "selftest_test": 3, "selftest_span": 1, "selftest_bit": 32},
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


# -- the march's written pattern, through the dump entry --------------------------------

SEEDS = (0, 0x1234ABCD)


def _dump_reference(grid, lds_words, seed, invert):
    from cro_amd.nodeops.probe import pattern_words

    return np.stack([pattern_words(b * lds_words, lds_words, seed, invert) for b in range(grid)])


@pytest.mark.parametrize("lds_bytes", [16, 1024, 4096 + 16])
@pytest.mark.parametrize("grid", [1, 3])
def test_march_writes_the_pattern_of_its_block_seed_and_pass(grid, lds_bytes):
    """What the kernel's fill left in LDS is cropattern.h's word of
    block * lds_words + offset, for both seeds and both passes; nothing was
    stored after the marched words."""
    _require_gpu()
    from cro_amd.nodeops.probe import compute_lds_dump

    lds_words = lds_bytes // 4
    dumps = {}
    for seed in SEEDS:
        for invert in (0, 1):
            got, guard_bad = compute_lds_dump(0, grid, lds_bytes, seed=seed, invert=invert)
            assert got.shape == (grid, lds_words) and got.dtype == np.uint32
            want = _dump_reference(grid, lds_words, seed, invert)
            assert np.array_equal(got, want), (seed, invert, np.flatnonzero(got != want)[:8])
            assert guard_bad == 0, (seed, invert, guard_bad)
            dumps[seed, invert] = got
    # a constant base, an ignored seed or an uncomplemented second pass would
    # have to fail above: the references themselves differ
    assert not np.array_equal(dumps[SEEDS[0], 0], dumps[SEEDS[1], 0])
    assert np.array_equal(dumps[SEEDS[0], 1], ~dumps[SEEDS[0], 0])
    if grid == 3:
        blocks = dumps[SEEDS[0], 0]
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert not np.array_equal(blocks[a], blocks[b])


def test_march_writes_the_pattern_over_a_whole_cu():
    """163840 bytes, two workgroups: every word of both, and no room for a
    guard."""
    _require_gpu()
    from cro_amd.nodeops.probe import compute_lds_dump

    lds_words = FULL_LDS // 4
    for seed, invert in ((SEEDS[1], 0), (SEEDS[0], 1)):
        got, guard_bad = compute_lds_dump(0, 2, FULL_LDS, seed=seed, invert=invert)
        want = _dump_reference(2, lds_words, seed, invert)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        assert guard_bad == 0
        assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("invert", [0, 1])
def test_dump_shows_a_plant_in_exactly_its_words(invert):
    """Span 5 from word 2: words 2..6, across the boundary of vectors 0 and 1."""
    _require_gpu()
    from cro_amd.nodeops.probe import compute_lds_dump

    bit, elem, span = 7, 2, 5
    got, guard_bad = compute_lds_dump(0, 3, 1024, seed=SEEDS[1], invert=invert,
                                      plant_elem=elem, plant_span=span, plant_bit=bit)
    diff = got ^ _dump_reference(3, 256, SEEDS[1], invert)
    want = np.zeros_like(diff)
    want[:, elem:elem + span] = 1 << bit
    assert np.array_equal(diff, want), np.argwhere(diff != want)[:8]
    assert guard_bad == 0


def test_dump_refuses_bad_arguments():
    _require_gpu()
    from cro_amd.nodeops.probe import compute_lds_dump

    for kw in ({"grid_blocks": 0}, {"grid_blocks": 9}, {"lds_bytes": 0}, {"lds_bytes": 24},
               {"lds_bytes": FULL_LDS + 16}, {"plant_elem": 256, "plant_span": 1},
               {"plant_elem": 255, "plant_span": 2}, {"plant_span": 1, "plant_bit": 32}):
        args = dict({"grid_blocks": 1, "lds_bytes": 1024}, **kw)
        with pytest.raises(RuntimeError, match="rc=-10"):
            compute_lds_dump(0, **args)


# -- self-test mode 3: real LDS plants on every workgroup -------------------------------


def _plants(lds_bytes):
    """(name, first word, span) of the plants a size has room for."""
    words = lds_bytes // 4
    out = [("word0", 0, 1), ("last", words - 1, 1)]
    if words >= 5:
        out.append(("vectors", 3, 2))  # words 3-4: vectors 0 and 1
    if words >= 65 * 4:
        out.append(("waves", 63 * 4 + 3, 2))  # vectors 63-64: waves 0 and 1
    if words >= 257 * 4:
        out.append(("trips", 255 * 4 + 3, 2))  # vectors 255-256: wave 3, then wave 0's second trip
    if lds_bytes == 1024:
        out.append(("all", 0, words))
    return out


MODE3 = [(lds_bytes, name, elem, span) for lds_bytes in (16, 1024, 4096 + 16, FULL_LDS)
         for name, elem, span in _plants(lds_bytes)]


def _mismatch_message(res, records, first):
    from cro_amd.nodeops.probe import decode_location

    loc = decode_location(int(records["xcc_id"][first]), int(records["hw_id"][first]))
    return (
        f"compute mismatch in {res['failed_test']} at xcd={loc['xcd']} se={loc['se']} "
        f"sh={loc['sh']} cu={loc['cu']} simd={loc['simd']}: element {records['first_bad'][first]}, "
        f"bits 0x{records['bits_bad'][first]:08x}; {res['waves_bad']} of {res['waves_run']} "
        f"waves bad on {res['cus_bad']} CUs"
    )


@pytest.mark.parametrize("bit", [3, 31])
@pytest.mark.parametrize("sel_pass", [0, 1, 2])
@pytest.mark.parametrize("lds_bytes,name,elem,span", MODE3)
def test_lds_plant_is_flagged_by_the_waves_that_verify_it(lds_bytes, name, elem, span, sel_pass,
                                                          bit):
    """Words made wrong in LDS itself, by another wave, between fill and
    verify: the clean run's verify loop must count each once per selected pass
    and iteration, on the wave that owns it, and name the lowest."""
    _require_gpu()
    from cro_amd.nodeops.probe import lds_plant_per_wave, run_compute_records

    iters = 2
    res, records = run_compute_records(
        0, lds_bytes=lds_bytes, iters=iters, selftest_mode=3, selftest_test="lds",
        selftest_elem=elem, selftest_span=span, selftest_pass=sel_pass, selftest_bit=bit)
    counts, firsts = lds_plant_per_wave(elem, span)
    assert sum(counts) == span
    passes = 2 if sel_pass == 2 else 1
    wave = np.arange(len(records)) % 4
    want_n = np.array(counts, dtype=np.uint32)[wave] * passes * iters
    want_first = np.array(firsts, dtype=np.uint32)[wave]
    hit = want_n != 0
    assert res["rounds"] == 1 and len(records) == 4 * res["grid_blocks"] == 4 * res["cus_expected"]
    assert np.all(records["valid"] == 1)
    assert np.array_equal(records["fail_mask"], np.where(hit, 8, 0))
    assert np.array_equal(records["n_bad"], want_n)
    assert np.array_equal(records["first_bad"], want_first)
    assert np.array_equal(records["bits_bad"], np.where(hit, np.uint32(1 << bit), 0))
    first = int(np.flatnonzero(hit)[0])
    assert res["ok"] is False and res["rc"] == -30 and res["failed_test"] == "lds", res
    assert res["bad_lds"] == res["waves_bad"] == int(hit.sum()), res
    assert res["bad_f32"] == res["bad_i8"] == res["bad_bf16"] == 0, res
    assert res["first_bad_index"] == first and res["first_bad_record"] == first, res
    assert res["first_bad"] == firsts[first % 4] and res["bits_bad"] == 1 << bit, res
    assert res["n_bad"] == counts[first % 4] * passes * iters, res
    assert res["cus_bad"] == np.unique(_keys(records)[hit]).size == res["cus_seen"], res
    assert res["msg"] == _mismatch_message(res, records, first), res


# -- self-test mode 4: a real LDS plant on one CU -----------------------------------------


def test_lds_plant_is_located_on_its_cu():
    """The last word of a CU's whole LDS, on the workgroups of one CU: only
    that CU's wave 3 (vector 10239 = 39 * 256 + 255) may flag it."""
    _require_gpu()
    from cro_amd.nodeops.probe import decode_cu_key, lds_verify_wave, run_compute_records

    clean = _clean_default()[1]
    key = int(_keys(clean)[len(clean) // 3 + 2])
    last = FULL_LDS // 4 - 1
    assert lds_verify_wave(last) == 3
    opts = dict(iters=1, selftest_mode=4, selftest_test="lds", selftest_elem=last,
                selftest_span=1, selftest_pass=2, selftest_bit=30)
    res, records = run_compute_records(0, selftest_key=key, **opts)
    on_cu = _keys(records) == key
    owner = np.arange(len(records)) % 4 == 3
    flagged = records["fail_mask"] != 0
    assert on_cu.any(), "the chosen CU ran no workgroup in this run"
    assert np.array_equal(flagged, on_cu & owner)
    assert np.all(records["fail_mask"][flagged] == 8)
    assert np.all(records["n_bad"][flagged] == 2) and not records["n_bad"][~flagged].any()
    assert np.all(records["first_bad"][flagged] == last)
    assert np.all(records["bits_bad"][flagged] == 1 << 30)
    assert res["ok"] is False and res["rc"] == -30 and res["failed_test"] == "lds", res
    assert res["cus_bad"] == 1 and res["bad_cu_keys"] == [key], res
    assert res["waves_bad"] == res["bad_lds"] == int(flagged.sum()), res
    assert res["first_bad"] == last and res["first_bad_index"] == int(np.flatnonzero(flagged)[0])
    assert {k: res[k] for k in ("xcd", "se", "sh", "cu")} == decode_cu_key(key), res
    # a key no CU has: nothing is planted, nothing flagged
    res, records = run_compute_records(0, selftest_key=key | (0xF << 20), **opts)
    assert res["ok"] is True and not records["fail_mask"].any(), res


# -- the per-wave tallies, through the caller's expected tiles ----------------------------

# element -> (lane, register) of the result maps (cromfma.h):
#   16x16: row * 16 + col is lane 16 * (row // 4) + col, register row % 4
#   32x32: row * 32 + col is lane 32 * ((row // 4) % 2) + col, register 4 * (row // 8) + row % 4
TALLY_CASES = {
    # the lowest element is not in the lowest lane
    "low_elem_high_lane": {"16": {16: 1 << 4, 1: 1 << 9},       # lane 0 reg 1; lane 1 reg 0
                           "32": {4 * 32: 1 << 4, 32 + 1: 1 << 9}},  # lane 32 reg 0; lane 1 reg 1
    # one lane, two registers
    "one_lane_two_regs": {"16": {8 * 16 + 5: 1 << 2, 10 * 16 + 5: 1 << 31},   # lane 37
                          "32": {5 * 32 + 13: 1 << 2, 21 * 32 + 13: 1 << 31}},  # lane 45
    # one register, lanes 0 and 63, different bits
    "lanes_0_and_63": {"16": {2 * 16: 1 << 0, 14 * 16 + 15: 1 << 17},      # register 2
                       "32": {9 * 32: 1 << 0, 13 * 32 + 31: 1 << 17}},   # register 5
}
TILE_TESTS = {"f32": ("mfma_f32", "16"), "i8": ("mfma_i8", "16"), "bf16": ("mfma_bf16", "32")}


def _altered_tile(kind, case, seed=0):
    """(tile to hand in, n_bad per iteration, first_bad, bits_bad), the last
    three derived from the two tiles alone."""
    from cro_amd.nodeops.probe import compute_expected_tiles

    clean = np.ascontiguousarray(compute_expected_tiles(seed)[kind])
    tile = clean.copy()
    bits = tile.view(np.uint32).reshape(-1)
    if case == "all":
        bits ^= np.uint32(1) << (np.arange(bits.size, dtype=np.uint32) % np.uint32(32))
    else:
        for elem, xor in TALLY_CASES[case][TILE_TESTS[kind][1]].items():
            bits[elem] ^= np.uint32(xor)
    diff = tile.view(np.uint32).reshape(-1) ^ clean.view(np.uint32).reshape(-1)
    bad = np.flatnonzero(diff)
    return tile, int(bad.size), int(bad[0]), int(np.bitwise_or.reduce(diff))


@pytest.mark.parametrize("case", list(TALLY_CASES) + ["all"])
@pytest.mark.parametrize("kind", ["f32", "i8", "bf16"])
def test_wave_tally_counts_values_and_names_the_lowest_element(kind, case):
    _require_gpu()
    from cro_amd.nodeops.probe import run_compute_records

    iters = 2
    tile, count, first, bits = _altered_tile(kind, case)
    if case == "all":
        assert count == tile.size and bits == 0xFFFFFFFF
    else:
        assert count == 2
    test = TILE_TESTS[kind][0]
    res, records = run_compute_records(0, tiles={kind: tile}, grid_blocks=8, iters=iters,
                                       max_rounds=1)
    assert len(records) == 32 and np.all(records["valid"] == 1)
    assert np.all(records["fail_mask"] == TEST_BITS[test])
    assert np.all(records["n_bad"] == count * iters), records["n_bad"]
    assert np.all(records["first_bad"] == first), records["first_bad"]
    assert np.all(records["bits_bad"] == bits), [hex(b) for b in records["bits_bad"]]
    assert res["rc"] == -30 and res["failed_test"] == test and res["waves_bad"] == 32, res
    assert (res["n_bad"], res["first_bad"], res["bits_bad"]) == (count * iters, first, bits), res
    # this call only: the cached tiles are whole
    assert run_compute_records(0, grid_blocks=8, iters=1, max_rounds=1)[0]["ok"] is True


def test_wave_tally_leads_with_the_lowest_failing_test():
    """f32 and bf16 altered together: the counts add up, element and bits are
    the f32 tile's, not a mixture."""
    _require_gpu()
    from cro_amd.nodeops.probe import run_compute_records

    iters = 2
    t32, n32, first32, bits32 = _altered_tile("f32", "one_lane_two_regs")
    t16, n16, first16, bits16 = _altered_tile("bf16", "low_elem_high_lane")
    assert first32 != first16 and bits32 != bits16
    res, records = run_compute_records(0, tiles={"f32": t32, "bf16": t16}, grid_blocks=8,
                                       iters=iters, max_rounds=1)
    assert np.all(records["fail_mask"] == 5)
    assert np.all(records["n_bad"] == (n32 + n16) * iters)
    assert np.all(records["first_bad"] == first32) and np.all(records["bits_bad"] == bits32)
    assert res["rc"] == -30 and res["failed_test"] == "mfma_f32", res
    assert res["bad_f32"] == res["bad_bf16"] == 32 and res["bad_i8"] == res["bad_lds"] == 0, res


def test_wave_tally_leads_with_bf16_over_a_planted_lds():
    """bf16 altered and every vector of the first trip planted (mode 3), so
    all four waves fail both: element and bits are bf16's."""
    _require_gpu()
    from cro_amd.nodeops.probe import lds_plant_per_wave, run_compute_records

    iters = 2
    t16, n16, first16, bits16 = _altered_tile("bf16", "lanes_0_and_63")
    counts, _ = lds_plant_per_wave(0, 1024)
    assert counts == [256] * 4
    res, records = run_compute_records(
        0, tiles={"bf16": t16}, grid_blocks=8, lds_bytes=4096 + 16, iters=iters, max_rounds=1,
        selftest_mode=3, selftest_test="lds", selftest_elem=0, selftest_span=1024,
        selftest_pass=1, selftest_bit=12)
    assert bits16 != 1 << 12
    assert np.all(records["fail_mask"] == 12)
    assert np.all(records["n_bad"] == (n16 + 256) * iters)
    assert np.all(records["first_bad"] == first16) and np.all(records["bits_bad"] == bits16)
    assert res["rc"] == -30 and res["failed_test"] == "mfma_bf16", res
    assert res["bad_bf16"] == res["bad_lds"] == 32, res


# -- host side ------------------------------------------------------------------------------


def test_seed_changes_rebuild_the_tiles():
    """Seed A, seed 0, seed A again: each upload gives the tiles the kernel's
    own inputs produce; after a change, mode 1 flips one element of the new
    seed's tile and of no stale one."""
    _require_gpu()
    from cro_amd.nodeops.probe import run_compute_records

    small = dict(grid_blocks=8, iters=1, max_rounds=1, lds_bytes=1024)
    for seed in (SEEDS[1], 0, SEEDS[1]):
        res, records = run_compute_records(0, seed=seed, **small)
        assert res["ok"] is True and not records["fail_mask"].any(), (seed, res)
        for test, elem, bit in MODE1[:3]:
            res, records = run_compute_records(0, seed=seed, selftest_mode=1, selftest_test=test,
                                               selftest_elem=elem, selftest_bit=bit, **small)
            assert res["rc"] == -30 and res["failed_test"] == test, (seed, res)
            assert np.all(records["fail_mask"] == TEST_BITS[test]), (seed, test)
            assert np.all(records["n_bad"] == 1) and np.all(records["first_bad"] == elem)
            assert np.all(records["bits_bad"] == 1 << bit)


def test_every_round_writes_its_own_records():
    """Eight workgroups never cover the device: all three rounds run, each
    into its own part of the record buffer."""
    _require_gpu()
    from cro_amd.nodeops.probe import run_compute_records

    res, records = run_compute_records(0, grid_blocks=8, max_rounds=3, iters=1, lds_bytes=1024)
    assert res["ok"] is True and res["rounds"] == 3, res
    assert len(records) == 96 == res["waves_run"] and np.all(records["valid"] == 1)
    assert not records["fail_mask"].any() and np.all(records["first_bad"] == 0xFFFFFFFF)


def test_record_buffer_regrows_and_is_reused():
    _require_gpu()
    from cro_amd.nodeops.probe import run_compute_records

    cus = _clean_default()[0]["cus_expected"]
    few = dict(grid_blocks=1, max_rounds=1, iters=1, lds_bytes=1024)
    res, records = run_compute_records(0, **few)
    assert res["ok"] is True and len(records) == 4, res
    res, records = run_compute_records(0, grid_blocks=cus + 44, max_rounds=4, iters=1)
    assert res["ok"] is True and len(records) == res["rounds"] * 4 * (cus + 44), res
    assert np.all(records["valid"] == 1) and not records["fail_mask"].any()
    res, records = run_compute_records(0, **few)
    assert res["ok"] is True and len(records) == 4 and np.all(records["valid"] == 1), res


def test_clean_run_on_one_vector_of_lds():
    """16 bytes: one vector; 255 threads fill nothing and 63 lanes of wave 0
    are past the end in the verify."""
    _require_gpu()
    from cro_amd.nodeops.probe import run_compute_records

    res, records = run_compute_records(0, lds_bytes=16, iters=2)
    assert res["ok"] is True and res["lds_bytes"] == 16 and res["waves_bad"] == 0, res
    assert np.all(records["valid"] == 1) and not records["n_bad"].any()


CONCURRENT_CHILD = """
import json, threading
from cro_amd.nodeops.probe import load_library, run_compute
load_library(required=True)
barrier = threading.Barrier(4)
results = [None] * 4
def worker(i):
    barrier.wait(timeout=60)
    results[i] = [run_compute(0, seed=1000 + i, grid_blocks=8 + i, iters=1 + i, max_rounds=1,
                              lds_bytes=1024 * (1 + i)) for _ in range(3)]
threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
for t in threads: t.start()
for t in threads: t.join()
print(json.dumps(results))
"""


def test_concurrent_compute_stages_on_one_device_are_serialised():
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
            assert (res["grid_blocks"], res["iters"], res["lds_bytes"], res["rounds"]) == (
                8 + i, 1 + i, 1024 * (1 + i), 1), (i, res)
            assert res["waves_run"] == 4 * (8 + i), (i, res)


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
