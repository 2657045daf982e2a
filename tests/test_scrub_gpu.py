"""GPU-marked tests of the scrub-on-detach stage on a real MI355X.

Everything compares exactly against numpy (``cro_amd.nodeops.scrub.scrub_report``)
— no tolerances.  The verify kernel is shown to detect by handing it buffers
with wrong words planted on the host before upload, the stage by its
self-test options (wrong data only, in bounds); nothing on the GPU is
provoked.

Shapes are one word either side of every boundary of the kernels' own tiling:
the 16-byte vector (4 words), the wave (64 vectors = 256 words), the
workgroup's unrolled span (4 x 256 vectors = 4096 words), a whole grid pass
(``grid_blocks`` spans) and, once, the production grid's pass of 16 MiB.  No
test holds more than ~100 MiB of VRAM.
"""

import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
NONE = (1 << 64) - 1
SPAN = 4096  # words a workgroup covers per trip


def _require_gpu():
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU (KFD) on this host")


# -- fill kernel ---------------------------------------------------------------------

FILL_SHAPES = [(n, 0) for n in (1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097)] + [
    (n, 2) for n in (8191, 8192, 8193, 2 * 8192 + 4096 + 5)
]


@pytest.mark.parametrize("fill_word", [0, 0xFFFFFFFF, 0xDEADBEEF])
@pytest.mark.parametrize("n_words,grid_blocks", FILL_SHAPES)
def test_fill_every_word_and_nothing_else(n_words, grid_blocks, fill_word):
    """scrub_fill raises when a guard band or a slack word changed."""
    _require_gpu()
    from cro_amd.nodeops.scrub import scrub_fill

    got = scrub_fill(0, n_words, fill_word, grid_blocks)
    assert got.shape == (n_words,)
    assert np.array_equal(got, np.full(n_words, fill_word, dtype=np.uint32))


def test_fill_one_word_past_a_production_grid_pass():
    _require_gpu()
    from cro_amd.nodeops.scrub import grid_pass_words, scrub_fill

    n_words = grid_pass_words() + 1
    assert n_words == 1024 * SPAN + 1
    got = scrub_fill(0, n_words, 0xDEADBEEF, 0)
    assert np.array_equal(got, np.full(n_words, 0xDEADBEEF, dtype=np.uint32))


# -- verify kernel -------------------------------------------------------------------

FILL = 0xDEADBEEF
BASE = (1 << 33) + 12  # first_bad is a 64-bit word index


def _check_verify(words, grid_blocks=0, fill=FILL):
    from cro_amd.nodeops.scrub import scrub_report, scrub_verify

    want = scrub_report(words, fill, BASE)
    got = scrub_verify(0, words, fill, BASE, grid_blocks)
    assert got == want
    return got


@pytest.mark.parametrize("n_words", [1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_verify_clean_buffer(n_words):
    """A read past n_words would meet 0xA5 guard bytes and count them."""
    _require_gpu()
    got = _check_verify(np.full(n_words, FILL, dtype=np.uint32))
    assert got == {"n_bad": 0, "first_bad": NONE, "bits_bad": 0}


def _planted(n_words, positions, xor=0x00010000):
    words = np.full(n_words, FILL, dtype=np.uint32)
    for k, pos in enumerate(positions):
        words[pos] ^= np.uint32(xor if isinstance(xor, int) else xor[k])
    return words


PLANTS = [
    # name, n_words, positions, grid_blocks
    ("word0", 4097, [0], 0),
    ("last_word", 4096, [4095], 0),
    ("tail1", 4097, [4096], 0),
    ("tail2", 4098, [4097], 0),
    ("tail3_each", 4099, [4096, 4097, 4098], 0),
    ("tail_only_buffer", 3, [2], 0),
    ("lane_40", 4096, [4 * 40 + 1], 0),  # lane >= 32: a 32-bit popcount drops it
    ("lane_63_of_wave_3", 4096, [4 * (3 * 64 + 63) + 3], 0),
    ("last_vector_of_span", 4096, [4092], 0),
    ("last_slot_first_lane", 4096, [3 * 1024], 0),
    ("second_grid_pass", 2 * SPAN + 9, [SPAN + 4 * 70 + 2], 1),
    ("third_pass_and_tail", 2 * SPAN + 9, [5, 2 * SPAN + 1, 2 * SPAN + 8], 1),
    ("second_block", 2 * SPAN, [SPAN + 17], 2),
    ("two_in_one_vector", 4096, [400, 402], 0),
    ("all_64_lanes_of_a_wave", 4096, [1024 + 256 + 4 * lane + (lane & 3) for lane in range(64)], 0),
]


@pytest.mark.parametrize("name,n_words,positions,grid_blocks", PLANTS, ids=[p[0] for p in PLANTS])
def test_verify_reports_planted_words(name, n_words, positions, grid_blocks):
    _require_gpu()
    # a different bit per planted word, so bits_bad shows every one was seen
    xor = [1 << (k % 32) for k in range(len(positions))]
    got = _check_verify(_planted(n_words, positions, xor), grid_blocks)
    assert got["n_bad"] == len(positions)
    assert got["first_bad"] == BASE + min(positions)


def test_verify_every_word_bad():
    _require_gpu()
    got = _check_verify(np.full(2 * SPAN + 3, 0xA5A5A5A5, dtype=np.uint32), grid_blocks=1, fill=0)
    assert got == {"n_bad": 2 * SPAN + 3, "first_bad": BASE, "bits_bad": 0xA5A5A5A5}


# -- the stage -----------------------------------------------------------------------


def _assert_data_clean(res):
    assert res["n_bad"] == 0 and res["bits_bad"] == 0 and res["first_bad_got"] == 0
    assert res["first_bad_byte"] == NONE


def test_run_scrub_chunks_and_accounting():
    _require_gpu()
    from cro_amd.nodeops.scrub import run_scrub

    res = run_scrub(0, max_bytes=96 * MIB + 4096, chunk_bytes=32 * MIB)
    assert res["ok"] and res["rc"] == 0 and res["msg"] == "ok", res
    assert res["bytes_target"] == 96 * MIB + 4096
    assert res["chunks"] == 4 and res["alloc_refusals"] == 0
    assert res["bytes_scrubbed"] == res["bytes_verified"] == res["bytes_target"]
    _assert_data_clean(res)
    assert res["vram_total"] > 0 and res["vram_free_before"] > 0
    assert res["fraction"] == res["bytes_scrubbed"] / res["vram_total"]
    for rate in ("fill_gbps", "verify_gbps", "census_gbps"):
        assert res[rate] > 0, rate
    assert res["t_total_ms"] >= res["t_alloc_ms"] >= 0


SELF_BYTES, SELF_CHUNK = 8 * MIB, 4 * MIB
SELF_WORDS = SELF_BYTES // 4


def _selftest(**opts):
    from cro_amd.nodeops.scrub import run_scrub

    return run_scrub(0, max_bytes=SELF_BYTES, chunk_bytes=SELF_CHUNK, **opts)


def test_selftest_planted_content_is_seen_and_then_gone():
    _require_gpu()
    res = _selftest(selftest_mode=3, fill_word=0)
    assert res["ok"], res
    assert res["dirty_words_before"] == SELF_WORDS
    assert res["bytes_scrubbed"] == res["bytes_verified"] == SELF_BYTES
    _assert_data_clean(res)


def test_selftest_unfilled_content_fails_as_residue():
    _require_gpu()
    res = _selftest(selftest_mode=2, fill_word=0)
    assert not res["ok"] and res["rc"] == -40, res
    assert res["n_bad"] == SELF_WORDS and res["dirty_words_before"] == SELF_WORDS
    assert res["first_bad_byte"] == 0
    assert res["first_bad_got"] == 0xA5A5A5A5 and res["bits_bad"] == 0xA5A5A5A5
    assert res["bytes_scrubbed"] == 0 and res["bytes_verified"] == SELF_BYTES
    assert "residue" in res["msg"]


CHUNK_WORDS = SELF_CHUNK // 4


@pytest.mark.parametrize("bit", [0, 31])
@pytest.mark.parametrize("word", [0, CHUNK_WORDS - 1, CHUNK_WORDS, SELF_WORDS - 1])
@pytest.mark.parametrize("fill_word", [0, 0xDEADBEEF])
def test_selftest_one_flipped_bit_is_located(fill_word, word, bit):
    _require_gpu()
    res = _selftest(selftest_mode=1, selftest_word=word, selftest_bit=bit, fill_word=fill_word)
    assert not res["ok"] and res["rc"] == -40, res
    assert res["n_bad"] == 1
    assert res["first_bad_byte"] == 4 * word
    assert res["bits_bad"] == 1 << bit
    assert res["first_bad_got"] == fill_word ^ (1 << bit)
    assert res["bytes_verified"] == SELF_BYTES


@pytest.mark.parametrize("opts,what", [
    (dict(selftest_mode=1, selftest_word=SELF_WORDS), "selftest_word"),
    (dict(selftest_mode=1, selftest_bit=32), "selftest_bit"),
    (dict(selftest_mode=1, selftest_bit=-1), "selftest_bit"),
    (dict(selftest_mode=4), "selftest_mode"),
    (dict(min_fraction=1.5), "min_fraction"),
])
def test_bad_arguments(opts, what):
    _require_gpu()
    res = _selftest(**opts)
    assert not res["ok"] and res["rc"] == -1
    assert res["msg"] == f"bad argument: {what}"


def test_pretended_refusal_halves_the_request():
    _require_gpu()
    res = _selftest(selftest_refuse_at=2)
    assert res["ok"], res
    assert res["alloc_refusals"] == 1 and res["chunks"] == 3
    assert res["bytes_scrubbed"] == res["bytes_verified"] == res["bytes_target"] == SELF_BYTES
    _assert_data_clean(res)


def test_nothing_to_scrub_when_the_reserve_exceeds_free_memory():
    _require_gpu()
    from cro_amd.nodeops.scrub import run_scrub

    res = run_scrub(0, reserve_bytes=1 << 50)
    assert not res["ok"] and res["rc"] == -1 and res["bytes_target"] == 0
    assert res["msg"].startswith("nothing to scrub")
    assert res["chunks"] == 0


def test_fraction_floor():
    _require_gpu()
    from cro_amd.nodeops.scrub import run_scrub

    res = run_scrub(0, max_bytes=16 * MIB, min_fraction=0.999)
    assert not res["ok"] and res["rc"] == -41, res
    assert res["bytes_scrubbed"] == res["bytes_verified"] == 16 * MIB
    _assert_data_clean(res)
    assert "below floor" in res["msg"]


def test_bad_device_ordinal():
    _require_gpu()
    from cro_amd.nodeops.scrub import run_scrub

    res = run_scrub(4096, max_bytes=MIB)
    assert not res["ok"] and res["rc"] == -1 and "out of range" in res["msg"]


def test_two_threads_on_one_device():
    _require_gpu()
    import threading

    from cro_amd.nodeops.scrub import load_scrub_library, run_scrub

    load_scrub_library(required=True)
    barrier = threading.Barrier(2)
    results = [None, None]

    def worker(i):
        barrier.wait(timeout=60)
        results[i] = run_scrub(0, max_bytes=16 * MIB, chunk_bytes=4 * MIB, fill_word=i)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for res in results:
        assert res is not None and res["ok"], res
        assert res["chunks"] == 4 and res["bytes_verified"] == 16 * MIB


# -- life cycle and agent --------------------------------------------------------------


def test_lifecycle_scrubs_between_detach_start_and_detached():
    _require_gpu()
    from cro_amd.api.v1alpha1.types import Event
    from cro_amd.bench_harness import attach_detach_cycle, build_local_stack
    from cro_amd.nodeops.scrub import make_scrub_fn

    cdi_dir = os.path.join(os.environ.get("TMPDIR", "/tmp"), "cro-cdi-scrubtest")
    stack = build_local_stack(node_name="scrubtest", use_gpu=True, gpu_index=0, cdi_dir=cdi_dir)
    stack.ops.scrub_fn = make_scrub_fn(max_bytes=64 << 20)
    stack.mgr.start()
    try:
        attach_detach_cycle(stack, "scrub-e2e", size=1, timeout=180)
        assert stack.ops.cdi.devices("scrubtest") == []
        stack.mgr.recorder.flush()
        events = sorted(stack.mgr.client.list(Event), key=lambda e: e.first_seen)
        reasons = [e.reason for e in events]
        trail = [(e.reason, e.involved_name, e.message) for e in events]
        print(trail)
        assert "ScrubFailed" not in reasons, trail
        assert reasons.count("Scrubbed") == 1, trail
        assert (reasons.index("DetachStarted") < reasons.index("Scrubbed")
                < reasons.index("Detached")), reasons
        scrubbed = events[reasons.index("Scrubbed")]
        assert scrubbed.message.startswith("scrubbed 0.06 GiB ("), scrubbed.message
        assert ", verified; " in scrubbed.message
    finally:
        stack.mgr.stop()


def test_croagent_scrub():
    _require_gpu()
    from cro_amd.nodeops.scrub import run_scrub

    agent = os.path.join(REPO, "cro_amd", "agent", "croagent")
    assert os.path.exists(agent), "croagent not built (python -m cro_amd.hip.build)"
    proc = subprocess.run([agent, "scrub", "--device", "0", "--max-mib", "64"],
                          capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    data = json.loads(proc.stdout)
    assert data["ok"] is True and data["rc"] == 0
    assert data["bytes_scrubbed"] == data["bytes_verified"] == 64 * MIB
    assert list(data) == list(run_scrub(0, max_bytes=MIB))
    floor = subprocess.run([agent, "scrub", "--device", "0", "--max-mib", "16",
                            "--min-fraction", "0.999"],
                           capture_output=True, text=True, timeout=120)
    assert floor.returncode == 1
    assert json.loads(floor.stdout)["rc"] == -41
