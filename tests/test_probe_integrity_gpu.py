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


def _assert_integrity_ok(res, vram_bytes, link_bytes):
    from cro_amd.nodeops.probe import INTEGRITY_RATES, INTEGRITY_STAGES

    assert res["ok"], res
    assert res["rc"] == 0 and res["failed_stage"] == "" and res["n_bad"] == 0, res
    for stage in INTEGRITY_STAGES:
        assert res[f"{stage}_n_bad"] == 0, (stage, res)
    assert res["vram_passes"] == 2 and res["link_passes"] == 1, res
    assert res["vram_bytes_verified"] == vram_bytes * res["vram_passes"], res
    for stage in INTEGRITY_STAGES[1:]:
        assert res[f"{stage}_bytes_verified"] == link_bytes * res["link_passes"], (stage, res)
    for rate in INTEGRITY_RATES:
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
