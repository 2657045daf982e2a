"""GPU-marked tests of the deep (data-integrity) probe on a real MI355X.

Everything compares bit-exactly against the numpy reference
(``cro_amd.nodeops.probe.pattern_words``) — no tolerances.  The detector is
shown to detect by handing it buffers corrupted on the host before upload;
nothing on the GPU is provoked.

Shapes are the smallest that reach each way the kernels can go wrong: the
scalar tail, wave (64) and block (256) edges, an odd base, word indices past
2^32, and one size that makes the grid-stride loop iterate: the launch grid
is capped at 1024 workgroups x 256 lanes x 4 words = 2^20 words per pass, so
(1 << 22) + 7 words is four passes and a tail.

The driver (which chunk, seed, polarity and base the kernels are pointed at,
what a failure reports, the link floor, the cached pinned buffer) is tested
through the probe's self-test, further down: wrong data only, in bounds.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
NONE = (1 << 64) - 1

SHAPES = [
    (0, 1),
    (0, 3),  # tail only
    (0, 63),
    (0, 64),
    (0, 65),  # wave edge
    (7, 256 * 4 + 3),  # block edge plus tail, odd base
    ((1 << 32) - 5, 37),  # index crosses 32 bits
    ((1 << 36) + 1, 1027),
    (0, (1 << 22) + 7),  # 4 grid passes + tail
]
SEED = 0x1234ABCD


def _require_gpu():
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU (KFD) on this host")


_ref_cache = {}


def _ref(base, n, seed, invert):
    """Reference words, computed once per case and handed out read-only."""
    from cro_amd.nodeops.probe import pattern_words

    key = (base, n, seed, int(bool(invert)))
    if key not in _ref_cache:
        words = pattern_words(base, n, seed, invert)
        words.setflags(write=False)
        _ref_cache[key] = words
    return _ref_cache[key]


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("base,n", SHAPES)
def test_fill_matches_numpy(base, n, invert):
    _require_gpu()
    from cro_amd.nodeops.probe import pattern_fill

    got = pattern_fill(0, SEED, invert, base, n)
    assert np.array_equal(got, _ref(base, n, SEED, invert))


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("base,n", SHAPES)
def test_verify_accepts_clean(base, n, invert):
    _require_gpu()
    from cro_amd.nodeops.probe import pattern_verify

    rep = pattern_verify(0, SEED, invert, base, _ref(base, n, SEED, invert))
    assert rep == {"n_bad": 0, "first_bad": NONE, "bits_bad": 0}


# base 7, 256*4+3 words: vectors cover words 0..1023, words 1024..1026 are tail
_ONE_BASE, _ONE_N = 7, 256 * 4 + 3


@pytest.mark.parametrize(
    "index,bit",
    [(0, 0), (_ONE_N - 1, 31), (_ONE_N - 2, 5), (64, 17), (255, 1), (256, 30)],
)
def test_verify_detects_single_bit(index, bit):
    _require_gpu()
    from cro_amd.nodeops.probe import pattern_verify

    words = _ref(_ONE_BASE, _ONE_N, SEED, 0).copy()
    words[index] ^= np.uint32(1 << bit)
    rep = pattern_verify(0, SEED, 0, _ONE_BASE, words)
    assert rep == {"n_bad": 1, "first_bad": _ONE_BASE + index, "bits_bad": 1 << bit}


def test_verify_detects_spread_corruption():
    """17 bad words over several waves and blocks; a word's lane is
    (index // 4) % 64, so indices with (index // 4) % 64 >= 32 sit in the
    upper half of a wave."""
    _require_gpu()
    from cro_amd.nodeops.probe import pattern_verify

    base, n = (1 << 32) - 5, 8 * 1024 + 2
    indices = [
        5, 130, 131, 255, 256, 1023, 1024, 1500, 2047,
        2048, 3000, 4095, 4097, 6000, 8191, 8192, 8193,
    ]
    assert len(indices) == 17 and len(set(indices)) == 17
    assert sum(1 for i in indices if (i // 4) % 64 >= 32) >= 5
    assert len({i // 1024 for i in indices}) >= 5  # 1024 words per block
    words = _ref(base, n, SEED, 1).copy()
    want_bits = 0
    for k, i in enumerate(indices):
        flip = (1 << (k % 32)) | (1 << ((3 * k + 7) % 32))
        words[i] ^= np.uint32(flip)
        want_bits |= flip
    rep = pattern_verify(0, SEED, 1, base, words)
    assert rep == {"n_bad": 17, "first_bad": base + min(indices), "bits_bad": want_bits}


def test_verify_wrong_seed_counts_every_word():
    """Every word differs (the mix is a bijection), so every lane of every
    wave ballots 1: a 32-bit popcount of the 64-lane ballot would report
    about half of 4099."""
    _require_gpu()
    from cro_amd.nodeops.probe import pattern_verify

    n = 4099
    rep = pattern_verify(0, SEED ^ 0x1, 0, 0, _ref(0, n, SEED, 0))
    assert rep["n_bad"] == n
    assert rep["first_bad"] == 0


def test_verify_wrong_polarity():
    _require_gpu()
    from cro_amd.nodeops.probe import pattern_verify

    base, n = 7, 256 * 4 + 3
    rep = pattern_verify(0, SEED, 1, base, _ref(base, n, SEED, 0))
    assert rep == {"n_bad": n, "first_bad": base, "bits_bad": 0xFFFFFFFF}


def _assert_integrity_ok(res, vram_bytes, link_bytes, rates=True):
    from cro_amd.nodeops.probe import INTEGRITY_RATES, INTEGRITY_STAGES

    assert res["ok"], res
    assert res["rc"] == 0 and res["failed_stage"] == "" and res["n_bad"] == 0, res
    for stage in INTEGRITY_STAGES:
        assert res[f"{stage}_n_bad"] == 0, (stage, res)
    assert res["vram_passes"] == 2 and res["link_passes"] == 1, res
    assert res["vram_bytes_verified"] == vram_bytes * res["vram_passes"], res
    for stage in INTEGRITY_STAGES[1:]:
        assert res[f"{stage}_bytes_verified"] == link_bytes * res["link_passes"], (stage, res)
    for rate in INTEGRITY_RATES if rates else ():
        assert res[rate] > 0, (rate, res)


def test_run_integrity_end_to_end():
    _require_gpu()
    from cro_amd.nodeops.probe import run_integrity

    first = run_integrity(0, vram_bytes=64 * MIB, link_bytes=16 * MIB, seed=SEED)
    _assert_integrity_ok(first, 64 * MIB, 16 * MIB)
    assert first["vram_chunks"] == 1
    # second call: cached context (pinned buffer, events, report word)
    second = run_integrity(0, vram_bytes=64 * MIB, link_bytes=16 * MIB, seed=SEED + 1)
    _assert_integrity_ok(second, 64 * MIB, 16 * MIB)


def test_run_integrity_odd_span_covered_exactly():
    """3 MiB + 20 bytes in 1 MiB chunks: four chunks, the last of 5 words
    (one vector and one tail word)."""
    _require_gpu()
    from cro_amd.nodeops.probe import run_integrity

    span = 3 * MIB + 20
    res = run_integrity(0, vram_bytes=span, link_bytes=MIB + 20, seed=SEED, chunk_bytes=MIB)
    _assert_integrity_ok(res, span, MIB + 20)
    assert res["vram_chunks"] == 4


# -- the driver: each stage detects, locates and reports ---------------------------
#
# The self-test of the deep probe (croprobe.h) flips one bit of one word from
# the host between a stage's write and its compare; every access is in bounds
# and nothing on the GPU is provoked.  first_bad_got, the word the stage found,
# is compared with the numpy reference at the seed and polarity documented for
# that stage, which is what pins the per-chunk base (a chunk filled from base 0
# holds other words), the complement pass, the seed of the device→host stages
# and the polarity of the shader stages.

SPAN, CHUNK, LINK = 3 * MIB + 20, MIB, MIB + 20
V, C, L = SPAN // 4, CHUNK // 4, LINK // 4  # words: 4 chunks of C, C, C and 5
UPPER = 4 * 40 + 2  # vector 40 of its chunk: lane 40 of wave 0
assert V == 3 * C + 5 and L % 4 == 1 and (UPPER // 4) % 64 >= 32

VRAM_FLIPS = [
    (0, 0),
    (V - 1, 31),  # the span's last word: the single tail word of chunk 3
    (2 * C, 7),  # first word of chunk 2
    (3 * C - 1, 18),  # last word of chunk 2
    (3 * C, 1),  # chunk 3's one vector
    (C + UPPER, 24),  # chunk 1, upper half of a wave
]
LINK_FLIPS = [(0, 31), (L - 1, 0), (UPPER, 13)]  # L - 1 is a scalar-tail word
DETECTION = (
    [("vram", p, w, b) for p in (0, 1) for w, b in VRAM_FLIPS]
    + [(stage, 0, w, (b + 5 * k) % 32)
       for k, stage in enumerate(("h2d_dma", "d2h_dma", "h2d_kernel", "d2h_kernel"))
       for w, b in LINK_FLIPS]
)


def _stage_pattern(stage, vram_pass=0):
    """Seed and polarity of a stage as documented (integrity.hip, croprobe.h)."""
    seed = SEED ^ 0xA5A5A5A5 if stage.startswith("d2h") else SEED
    invert = vram_pass if stage == "vram" else int(stage.endswith("_kernel"))
    return seed, invert


def _assert_detected(res, stage, vram_pass, word, bit, vram_bytes, link_bytes):
    from cro_amd.nodeops.probe import INTEGRITY_STAGES, pattern_words

    seed, invert = _stage_pattern(stage, vram_pass)
    assert res["rc"] == -20 and res["ok"] is False, res
    assert res["failed_stage"] == stage, res
    assert res["n_bad"] == 1, res
    assert res["first_bad_byte"] == 4 * word, res
    assert res["bits_bad"] == 1 << bit, res
    want = int(pattern_words(word, 1, seed, invert)[0]) ^ (1 << bit)
    assert res["first_bad_got"] == want, (hex(res["first_bad_got"]), hex(want), res)
    assert res[f"{stage}_n_bad"] == 1, res
    at = INTEGRITY_STAGES.index(stage)
    span = {s: link_bytes for s in INTEGRITY_STAGES}
    span["vram"] = vram_bytes * 2
    for earlier in INTEGRITY_STAGES[:at]:
        assert res[f"{earlier}_bytes_verified"] == span[earlier], (earlier, res)
        assert res[f"{earlier}_n_bad"] == 0, (earlier, res)
    for later in INTEGRITY_STAGES[at + 1:]:
        assert res[f"{later}_bytes_verified"] == 0, (later, res)
        assert res[f"{later}_n_bad"] == 0, (later, res)
    if stage == "vram":
        assert res["vram_passes"] == vram_pass + 1, res
        assert res["vram_bytes_verified"] == vram_bytes * (vram_pass + 1), res
        assert res["link_passes"] == 0, res
    else:
        assert res["vram_passes"] == 2 and res["link_passes"] == 1, res
        assert res[f"{stage}_bytes_verified"] == link_bytes, res
    assert res["msg"] == (f"data mismatch in stage {stage}: 1 bad words, first at byte "
                          f"{4 * word}, bits 0x{1 << bit:08x}"), res


@pytest.mark.parametrize("stage,vram_pass,word,bit", DETECTION)
def test_stage_detects_locates_and_reports(stage, vram_pass, word, bit):
    _require_gpu()
    from cro_amd.nodeops.probe import run_integrity

    sizes = dict(vram_bytes=SPAN, chunk_bytes=CHUNK, link_bytes=LINK, seed=SEED)
    res = run_integrity(0, selftest_stage=stage, selftest_pass=vram_pass, selftest_word=word,
                        selftest_bit=bit, **sizes)
    _assert_detected(res, stage, vram_pass, word, bit, SPAN, LINK)
    assert res["vram_chunks"] == 4
    # nothing of the flip stays behind
    _assert_integrity_ok(run_integrity(0, **sizes), SPAN, LINK)


@pytest.mark.parametrize("stage,vram_pass", [("vram", 0), ("vram", 1), ("h2d_kernel", 0)])
def test_detects_in_a_later_grid_pass(stage, vram_pass):
    """One chunk of 20 MiB is five passes of the 1024-workgroup grid (2^20
    words each); word 2^22 + 3 is in the vector the fifth pass starts with."""
    _require_gpu()
    from cro_amd.nodeops.probe import run_integrity

    word, bit = (1 << 22) + 3, 9
    res = run_integrity(0, vram_bytes=20 * MIB, chunk_bytes=20 * MIB, link_bytes=20 * MIB,
                        seed=SEED, selftest_stage=stage, selftest_pass=vram_pass,
                        selftest_word=word, selftest_bit=bit)
    assert res["vram_chunks"] == 1
    _assert_detected(res, stage, vram_pass, word, bit, 20 * MIB, 20 * MIB)


def test_size_edges_clean():
    _require_gpu()
    from cro_amd.nodeops.probe import run_integrity

    # bytes that are no whole word are left out
    res = run_integrity(0, vram_bytes=SPAN + 2, link_bytes=LINK + 3, seed=SEED, chunk_bytes=MIB)
    _assert_integrity_ok(res, SPAN, LINK)
    assert res["vram_bytes_verified"] == 2 * (3 * MIB + 20) and res["vram_chunks"] == 4
    # chunk_bytes below one vector is one vector: six of them and a tail word
    res = run_integrity(0, vram_bytes=100, link_bytes=100, seed=SEED, chunk_bytes=5)
    _assert_integrity_ok(res, 100, 100, rates=False)
    assert res["vram_chunks"] == 7
    # one word in all
    res = run_integrity(0, vram_bytes=4, link_bytes=4, seed=SEED)
    _assert_integrity_ok(res, 4, 4, rates=False)
    assert res["vram_chunks"] == 1
    # chunk_bytes that is no multiple of 16 is rounded down
    res = run_integrity(0, vram_bytes=SPAN, link_bytes=LINK, seed=SEED, chunk_bytes=MIB + 7)
    _assert_integrity_ok(res, SPAN, LINK)
    assert res["vram_chunks"] == 4


@pytest.mark.parametrize("vram_pass", [0, 1])
def test_detects_in_a_last_chunk_that_is_one_tail_word(vram_pass):
    _require_gpu()
    from cro_amd.nodeops.probe import run_integrity

    res = run_integrity(0, vram_bytes=100, link_bytes=100, seed=SEED, chunk_bytes=5,
                        selftest_stage="vram", selftest_pass=vram_pass, selftest_word=24,
                        selftest_bit=30)
    assert res["vram_chunks"] == 7
    _assert_detected(res, "vram", vram_pass, 24, 30, 100, 100)


def _child(code, timeout):
    """Run ``code`` in a fresh interpreter with a time limit of its own; the
    last line it prints is JSON."""
    proc = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True,
                          text=True, timeout=timeout)
    assert proc.returncode == 0, (proc.returncode, proc.stdout[-2000:], proc.stderr[-2000:])
    return json.loads(proc.stdout.strip().splitlines()[-1])


PINNED_CHILD = """
import json
from cro_amd.nodeops.probe import run_integrity
MIB = 1 << 20
def run(link, **kw):
    return run_integrity(0, vram_bytes=MIB, link_bytes=link, seed=%d, **kw)
out = [run(MIB), run(4 * MIB + 20), run(MIB)]
for stage in ("d2h_kernel", "h2d_dma"):
    out.append(run(MIB, selftest_stage=stage, selftest_word=MIB // 4 - 1, selftest_bit=3))
print(json.dumps(out))
""" % SEED


def test_pinned_buffer_regrow_and_reuse():
    """A fresh process, so the cached pinned buffer starts at 1 MiB: a larger
    link_bytes reallocates it, a smaller one afterwards reuses the larger
    buffer, and then the span is this call's, not the buffer's."""
    _require_gpu()
    first, grown, reused, bad_d2h, bad_h2d = _child(PINNED_CHILD, timeout=120)
    _assert_integrity_ok(first, MIB, MIB)
    _assert_integrity_ok(grown, MIB, 4 * MIB + 20)
    _assert_integrity_ok(reused, MIB, MIB)
    _assert_detected(bad_d2h, "d2h_kernel", 0, MIB // 4 - 1, 3, MIB, MIB)
    _assert_detected(bad_h2d, "h2d_dma", 0, MIB // 4 - 1, 3, MIB, MIB)
    assert bad_d2h["first_bad_byte"] == MIB - 4 == bad_h2d["first_bad_byte"]


# -- the link floor and the arguments -------------------------------------------------

SMALL = dict(vram_bytes=MIB, link_bytes=MIB, seed=SEED)


def test_link_floor_gate():
    _require_gpu()
    from cro_amd.nodeops.probe import INTEGRITY_STAGES, run_integrity

    # above any link: fails at the first link stage, after every data gate
    res = run_integrity(0, link_floor_gbps=1e9, **SMALL)
    assert res["rc"] == -21 and res["ok"] is False, res
    assert res["failed_stage"] == "h2d_dma", res
    assert res["n_bad"] == 0 and res["first_bad_got"] == 0, res
    assert res["vram_bytes_verified"] == 2 * MIB, res
    for stage in INTEGRITY_STAGES:
        assert res[f"{stage}_n_bad"] == 0, (stage, res)
        assert res[f"{stage}_bytes_verified"] > 0, (stage, res)
    for stage in INTEGRITY_STAGES[1:]:
        assert res[f"{stage}_bytes_verified"] == MIB, (stage, res)
    assert res["msg"] == (f"link rate {res['h2d_dma_gbps']:.1f} GB/s in stage h2d_dma below "
                          f"floor {1e9:.1f} GB/s"), res
    # below any link
    _assert_integrity_ok(run_integrity(0, link_floor_gbps=1e-6, **SMALL), MIB, MIB)


@pytest.mark.parametrize("link_bytes", [MIB, 16 * MIB, 64 * MIB])
def test_link_floor_is_held_against_every_link_stage(link_bytes):
    """Floors between the four rates of a first run, so that stages pass before
    one that fails whenever h2d_dma is not the slowest.  Which of the four is
    depends on the size: on an MI355X the copy engine's set-up time makes
    h2d_dma the slowest at 1 MiB (29 against 31, 36 and 47 GB/s) and at 64 MiB
    it is the fastest (56.3 against 55.8, 54.5 and 55.0 GB/s).  No rate is
    assumed: whatever a run measured, its verdict must follow from the rates it
    reports itself — ok only with all four at the floor or above, else -21
    naming the first stage below it, in the order of the stages."""
    _require_gpu()
    from cro_amd.nodeops.probe import INTEGRITY_STAGES, run_integrity

    links = INTEGRITY_STAGES[1:]
    sizes = dict(vram_bytes=MIB, link_bytes=link_bytes, seed=SEED)
    plain = run_integrity(0, **sizes)
    _assert_integrity_ok(plain, MIB, link_bytes)
    rates = sorted(plain[f"{s}_gbps"] for s in links)
    for lo, hi in zip(rates, rates[1:]):
        floor = (lo + hi) / 2
        res = run_integrity(0, link_floor_gbps=floor, **sizes)
        below = [s for s in links if res[f"{s}_gbps"] < floor]
        for stage in INTEGRITY_STAGES:  # the floor comes after every data gate
            assert res[f"{stage}_n_bad"] == 0 and res[f"{stage}_bytes_verified"] > 0, res
        if not below:
            assert res["ok"] and res["rc"] == 0 and res["failed_stage"] == "", (floor, res)
            continue
        assert res["rc"] == -21 and res["ok"] is False, (floor, res)
        assert res["failed_stage"] == below[0], (floor, below, res)
        assert res["msg"] == (f"link rate {res[below[0] + '_gbps']:.1f} GB/s in stage "
                              f"{below[0]} below floor {floor:.1f} GB/s"), res


@pytest.mark.parametrize("stage", ["vram", "d2h_kernel"])
def test_data_gate_comes_before_link_floor(stage):
    _require_gpu()
    from cro_amd.nodeops.probe import run_integrity

    res = run_integrity(0, link_floor_gbps=1e9, selftest_stage=stage, selftest_word=77,
                        selftest_bit=4, **SMALL)
    _assert_detected(res, stage, 0, 77, 4, MIB, MIB)


BAD_OPTIONS = [
    ("link_floor_gbps", {"link_floor_gbps": float("nan")}),
    ("link_floor_gbps", {"link_floor_gbps": -1.0}),
    ("selftest_stage", {"selftest_stage": 6}),
    ("selftest_stage", {"selftest_stage": -1}),
    ("selftest_bit", {"selftest_stage": 1, "selftest_bit": 32}),
    ("selftest_bit", {"selftest_stage": 1, "selftest_bit": -1}),
    ("selftest_pass", {"selftest_stage": 1, "selftest_pass": 2}),
    ("selftest_pass", {"selftest_stage": 1, "selftest_pass": -1}),
    ("selftest_pass", {"selftest_stage": 2, "selftest_pass": 1}),  # a link stage has one pass
    ("selftest_pass", {"selftest_stage": 5, "selftest_pass": 1}),
    ("selftest_word", {"selftest_stage": 1, "selftest_word": MIB // 4}),  # first word past the span
    ("selftest_word", {"selftest_stage": 1, "selftest_pass": 1, "selftest_word": MIB // 4}),
    ("selftest_word", {"selftest_stage": 2, "selftest_word": MIB // 8}),
    ("selftest_word", {"selftest_stage": 3, "selftest_word": MIB // 8}),
    ("selftest_word", {"selftest_stage": 4, "selftest_word": MIB // 8}),
    ("selftest_word", {"selftest_stage": 5, "selftest_word": MIB // 8}),
    ("selftest_word", {"selftest_stage": 5, "selftest_word": (1 << 64) - 1}),
]


@pytest.mark.parametrize("field,opts", BAD_OPTIONS)
def test_bad_options_are_refused_before_anything_runs(field, opts):
    _require_gpu()
    from cro_amd.nodeops.probe import INTEGRITY_STAGES, run_integrity

    res = run_integrity(0, vram_bytes=MIB, link_bytes=MIB // 2, seed=SEED, **opts)
    assert res["rc"] == -1 and res["ok"] is False, res
    assert res["msg"] == f"bad argument: {field}", res
    assert res["vram_passes"] == 0 and res["link_passes"] == 0 and res["vram_chunks"] == 0, res
    for stage in INTEGRITY_STAGES:
        assert res[f"{stage}_bytes_verified"] == 0, (stage, res)


def test_last_word_of_each_span_is_accepted_and_ordinal_is_named_first():
    _require_gpu()
    from cro_amd.nodeops.probe import device_count, run_integrity

    # the bound of selftest_word is the stage's own span
    res = run_integrity(0, vram_bytes=MIB, link_bytes=MIB // 2, seed=SEED,
                        selftest_stage="vram", selftest_word=MIB // 4 - 1)
    _assert_detected(res, "vram", 0, MIB // 4 - 1, 0, MIB, MIB // 2)
    res = run_integrity(0, vram_bytes=MIB, link_bytes=MIB // 2, seed=SEED,
                        selftest_stage="d2h_dma", selftest_word=MIB // 8 - 1)
    _assert_detected(res, "d2h_dma", 0, MIB // 8 - 1, 0, MIB, MIB // 2)
    for device in (-1, device_count()):
        for opts in ({}, {"selftest_stage": 9}, {"link_floor_gbps": float("nan")}):
            res = run_integrity(device, **SMALL, **opts)
            assert res["rc"] == -1 and res["ok"] is False, res
            assert "out of range" in res["msg"], res


# -- raw entries: nothing written past n_words ---------------------------------------


@pytest.mark.parametrize("base,n", SHAPES)
def test_fill_leaves_slack_and_guard_untouched(base, n):
    _require_gpu()
    import ctypes

    from cro_amd.nodeops.probe import load_library

    lib = load_library(required=True)
    for invert in (0, 1):
        out = np.zeros(n, dtype=np.uint32)
        guard_ok = ctypes.c_int(-1)
        rc = lib.cro_probe_pattern_fill(0, SEED, invert, base, n,
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)),
                                        ctypes.byref(guard_ok))
        assert rc == 0 and guard_ok.value == 1, (rc, guard_ok.value)
        assert np.array_equal(out, _ref(base, n, SEED, invert))
    assert lib.cro_probe_pattern_fill(0, SEED, 0, base, n,
                                      out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)),
                                      None) == -10


# -- concurrency -------------------------------------------------------------------------

CONCURRENT_CHILD = """
import json, threading
from cro_amd.nodeops.probe import load_library, run_integrity
load_library(required=True)
MIB = 1 << 20
barrier = threading.Barrier(4)
results = [None] * 4
def worker(i):
    barrier.wait(timeout=60)
    results[i] = [run_integrity(0, 8 * MIB, 2 * MIB, seed=i) for _ in range(3)]
threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
for t in threads: t.start()
for t in threads: t.join()
print(json.dumps([r for per in results for r in (per or [])]))
"""


def test_concurrent_deep_probes_on_one_device_are_serialised():
    """Four reconcile workers on one device at once (ctypes releases the GIL):
    one context, whose pinned buffer, report word and events no two calls
    may share; the first of the calls sets it up."""
    _require_gpu()
    results = _child(CONCURRENT_CHILD, timeout=180)
    assert len(results) == 12
    for res in results:
        _assert_integrity_ok(res, 8 * MIB, 2 * MIB)


def test_croagent_probe_deep():
    _require_gpu()
    agent = os.path.join(REPO, "cro_amd", "agent", "croagent")
    assert os.path.exists(agent), "croagent not built (python -m cro_amd.hip.build)"
    argv = [agent, "probe", "--device", "0"]
    deep = subprocess.run(
        argv + ["--deep", "--vram-mib", "64", "--link-mib", "16"],
        capture_output=True, text=True, timeout=120,
    )
    assert deep.returncode == 0, deep.stdout + deep.stderr
    out = json.loads(deep.stdout)
    assert out["ok"] is True and out["integrity"]["ok"] is True, out
    assert out["integrity"]["vram_bytes_verified"] == 2 * 64 * MIB
    quick = subprocess.run(argv, capture_output=True, text=True, timeout=120)
    assert quick.returncode == 0, quick.stdout + quick.stderr
    assert "integrity" not in json.loads(quick.stdout)


def test_deep_lifecycle_real_node_path():
    """One attach→detach with the deep probe as the node-ops hook."""
    _require_gpu()
    from cro_amd.api.v1alpha1.types import Event
    from cro_amd.bench_harness import attach_detach_cycle, build_local_stack
    from cro_amd.nodeops.probe import make_probe_fn

    cdi_dir = os.path.join(os.environ.get("TMPDIR", "/tmp"), "cro-cdi-deeptest")
    stack = build_local_stack(node_name="deeptest", use_gpu=True, gpu_index=0, cdi_dir=cdi_dir)
    stack.ops.probe_fn = make_probe_fn("deep", vram_bytes=64 * MIB, link_bytes=16 * MIB)
    stack.mgr.start()
    try:
        attach_detach_cycle(stack, "deep-e2e", size=1, timeout=180)
        assert stack.ops.cdi.devices("deeptest") == []
        stack.mgr.recorder.flush()
        online = [e for e in stack.mgr.client.list(Event) if e.reason == "Online"]
        assert online and "integrity: vram 0.06 GiB" in online[-1].message, online
    finally:
        stack.mgr.stop()
