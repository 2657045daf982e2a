"""CPU tests of the quick probe (cro_amd/hip/probe.hip): the two C structs
against their ctypes mirrors, the numpy references the GPU tests compare with
(``fmaf_chain`` against a true ``fmaf`` chain and the header's, the closed
form of the bf16 rate kernel's operands), the code the compiler emits for the
two matrix kernels, and the Python plumbing of the probe options.

The inputs of the exact f32 GPU tests are made here (``f32_cases``) so that
this file can show, without a GPU, that the numpy reference is the true chain
for every one of them: no step of any of them falls on a rounding tie.
"""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cro_amd.hip import build as hip_build
from cro_amd.nodeops import probe as probe_mod

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(REPO, "cro_amd", "hip")

RANDOM_KS = (4, 8, 12, 64, 128, 1024)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# -- inputs of the exact f32 tile tests (shared with test_probe_quick_gpu.py) --------


def f32_cases():
    """name → (A 16xK, B Kx16), float32.  No NaNs: payloads are not specified."""
    cases = {}
    for k in RANDOM_KS:  # one K step, two, three (odd count), the probe's, long chains
        rng = np.random.default_rng(7000 + k)
        cases[f"normal_k{k}"] = (rng.standard_normal((16, k), dtype=np.float32),
                                 rng.standard_normal((k, 16), dtype=np.float32))
    for k in (4, 12):
        # small integers: exact whatever the rounding, so only the lane map
        # can make these differ; asymmetric, so a swapped index shows
        rng = np.random.default_rng(7100 + k)
        a = rng.integers(-9, 10, size=(16, k)).astype(np.float32)
        b = rng.integers(-9, 10, size=(k, 16)).astype(np.float32)
        cases[f"integers_k{k}"] = (a, b)
    # every product and every result is a float32 subnormal
    rng = np.random.default_rng(5)
    scale = np.float64(2.0) ** -70
    cases["subnormal_k8"] = ((rng.standard_normal((16, 8)) * scale).astype(np.float32),
                             (rng.standard_normal((8, 16)) * scale).astype(np.float32))
    # signed zeros: rows of +0 and of -0 against operands of both signs, and a
    # product that underflows to -0 and must stay -0 through steps of -0
    rng = np.random.default_rng(11)
    a = rng.standard_normal((16, 8), dtype=np.float32)
    b = rng.standard_normal((8, 16), dtype=np.float32)
    b[1:, :8] = -np.abs(b[1:, :8])
    b[1:, 8:] = np.abs(b[1:, 8:])
    a[3:] = -np.abs(a[3:])  # negative operands in the rows that stay non-zero
    a[0, :] = 0.0
    a[1, :] = -0.0
    a[2, :] = 0.0
    a[2, 0] = -np.float32(2.0) ** -100
    b[0, :] = np.float32(2.0) ** -100
    cases["signed_zeros_k8"] = (a, b)
    # cancellation: pairs x, -x along K against the same y, and one small
    # survivor.  k = 0, 1: a full-precision pair, of which a fused chain leaves
    # the rounding error of x * y behind (an unfused one leaves 0); k = 2: the
    # survivor, about 2^-30; k = 3, 4: a pair whose product float32 holds
    # exactly (12-bit operands), about 2^13 times the running sum, which it cuts
    # down to its own last place; k = 6, 5: a full-precision pair again, -x
    # first.  Any other order of the steps gives another result.  k = 7 adds 0.
    rng = np.random.default_rng(21)  # a seed without a tie step (asserted below)
    x = rng.standard_normal((16, 3), dtype=np.float32)
    y = rng.standard_normal((3, 16), dtype=np.float32)
    for m in (x[:, 1], y[1]):
        m.view(np.uint32)[...] &= np.uint32(0xFFFFF000)
        m *= np.float32(2.0) ** -6
    x[:, 2] *= np.float32(2.0) ** -8
    y[2] *= np.float32(2.0) ** -8
    a = np.zeros((16, 8), dtype=np.float32)
    b = rng.standard_normal((8, 16), dtype=np.float32)
    for j, (plus, minus) in enumerate(((0, 1), (3, 4), (6, 5))):
        a[:, plus], a[:, minus] = x[:, j], -x[:, j]
        b[plus] = b[minus] = y[j]
    a[:, 2] = rng.standard_normal(16, dtype=np.float32) * np.float32(2.0) ** -30
    cases["cancellation_k8"] = (a, b)
    return cases


# -- host programs ------------------------------------------------------------------


def _host_cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    pytest.fail("no host C++ compiler (c++/g++/clang++) on PATH")


def _build(tmp_path, name, source):
    src = tmp_path / f"{name}.cpp"
    src.write_text(source)
    exe = tmp_path / name
    subprocess.run(
        [_host_cxx(), "-std=c++17", "-O1", "-ffp-contract=off", f"-I{HIP_DIR}", str(src),
         "-o", str(exe)],
        check=True, capture_output=True, text=True,
    )
    return str(exe)


# -- structs ------------------------------------------------------------------------

MIRRORS = {"CroProbeResult": probe_mod.CroProbeResult, "CroProbeOpts": probe_mod.CroProbeOpts}


def _struct_main():
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "croprobe.h"', "int main() {"]
    for cname, mirror in MIRRORS.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for field, _ in mirror._fields_:
            lines.append(
                f'  printf("{cname} {field} %zu %zu\\n", offsetof({cname}, {field}), '
                f"sizeof((({cname}*)0)->{field}));"
            )
    lines += ["  return 0;", "}"]
    return "\n".join(lines)


def test_quick_struct_layout_matches_ctypes(tmp_path):
    """Every field the ctypes mirrors name exists in the header at the same
    offset and size, and the totals agree (so the header has no extra one)."""
    exe = _build(tmp_path, "struct_main", _struct_main())
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        parts = line.split()
        mirror = MIRRORS[parts[0]]
        if parts[1] == "sizeof":
            assert ctypes.sizeof(mirror) == int(parts[2]), line
        else:
            desc = getattr(mirror, parts[1])
            assert (desc.offset, desc.size) == (int(parts[2]), int(parts[3])), line
        seen += 1
    assert seen == len(MIRRORS) + sum(len(m._fields_) for m in MIRRORS.values())
    for mirror in MIRRORS.values():  # no padding holes
        end = 0
        for field, _ in mirror._fields_:
            desc = getattr(mirror, field)
            assert desc.offset == end, (mirror.__name__, field)
            end = desc.offset + desc.size
        assert end == ctypes.sizeof(mirror)
    assert ctypes.sizeof(probe_mod.CroProbeOpts) == 32
    zero = probe_mod._probe_opts()
    assert bytes(zero) == bytes(ctypes.sizeof(zero))  # every default is 0


# -- fmaf_chain ---------------------------------------------------------------------

# argv: "chain K" — a true fmaf chain, row-major A 16xK then B Kx16 as uint32
# bit patterns on stdin; "header" — the same through cro_cov_ref_f32 (K = 64).
CHAIN_MAIN = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "crocoverage.h"

int main(int argc, char** argv) {
  const bool header = argc == 2 && !strcmp(argv[1], "header");
  if (!header && !(argc == 3 && !strcmp(argv[1], "chain"))) return 2;
  const int K = header ? CRO_COV_F32_K : atoi(argv[2]);
  std::vector<float> A(16 * K), B(K * 16), D(256);
  for (std::vector<float>* m : {&A, &B})
    for (float& v : *m) {
      unsigned u;
      if (scanf("%u", &u) != 1) return 3;
      memcpy(&v, &u, 4);
    }
  if (header) {
    cro_cov_ref_f32(A.data(), B.data(), D.data());
  } else {
    for (int r = 0; r < 16; ++r)
      for (int c = 0; c < 16; ++c) {
        float acc = 0.f;
        for (int k = 0; k < K; ++k) acc = fmaf(A[r * K + k], B[k * 16 + c], acc);
        D[r * 16 + c] = acc;
      }
  }
  for (float v : D) {
    unsigned u;
    memcpy(&u, &v, 4);
    printf("%u\n", u);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def chain_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("chain"), "chain_main", CHAIN_MAIN)


def _host_chain(exe, a, b, header=False):
    text = " ".join(str(int(v)) for v in np.concatenate([_bits(a).ravel(), _bits(b).ravel()]))
    argv = [exe, "header"] if header else [exe, "chain", str(a.shape[1])]
    out = subprocess.run(argv, input=text, check=True, capture_output=True, text=True).stdout
    return np.array([int(v) for v in out.split()], dtype=np.uint32).reshape(16, 16)


@pytest.fixture(scope="module")
def cases():
    made = f32_cases()
    for a, b in made.values():
        a.setflags(write=False)
        b.setflags(write=False)
    return made


def test_f32_cases_are_what_the_gpu_tests_need(cases):
    assert RANDOM_KS == (4, 8, 12, 64, 128, 1024)
    for name, (a, b) in cases.items():
        k = a.shape[1]
        assert a.dtype == b.dtype == np.float32 and a.shape == (16, k) and b.shape == (k, 16)
        assert np.isfinite(a).all() and np.isfinite(b).all(), name
    for k in (4, 12):
        a, b = cases[f"integers_k{k}"]
        assert np.abs(a).max() <= 9 and np.abs(b).max() <= 9
        assert not np.array_equal(a[:k, :k], a[:k, :k].T)
        assert not np.array_equal(b[:k, :k], b[:k, :k].T)
        want, _ = probe_mod.fmaf_chain(a, b)
        assert np.array_equal(want, a.astype(np.int64) @ b.astype(np.int64))
        assert not np.array_equal(want, want.T)
    tiny = np.float32(2.0) ** -126  # smallest normal
    a, b = cases["subnormal_k8"]
    want, _ = probe_mod.fmaf_chain(a, b)
    assert (np.abs(want) < tiny).all() and (want != 0).all()  # all 256 subnormal, none lost
    prods = a[:, :, None].astype(np.float64) * b[None, :, :].astype(np.float64)
    assert (np.abs(prods) < tiny).all() and (prods != 0).all()
    a, b = cases["signed_zeros_k8"]
    want = _bits(probe_mod.fmaf_chain(a, b)[0])
    assert (want[0] == 0).all() and (want[1] == 0).all()  # +0 rows
    assert (want[2, :8] == 0x80000000).all() and (want[2, 8:] == 0).all()  # -0 kept / lost
    assert ((want[3:] & 0x7FFFFFFF) != 0).all()
    a, b = cases["cancellation_k8"]
    want, _ = probe_mod.fmaf_chain(a, b)
    # an unfused multiply-add (the product rounded first) and the same steps
    # in the opposite order both give other bits almost everywhere
    unfused = np.zeros((16, 16), dtype=np.float32)
    for k in range(8):
        unfused = unfused + a[:, k : k + 1] * b[k : k + 1, :]
    assert unfused.dtype == np.float32
    assert np.count_nonzero(_bits(want) != _bits(unfused)) > 192
    backwards, _ = probe_mod.fmaf_chain(a[:, ::-1], b[::-1])
    assert np.count_nonzero(_bits(want) != _bits(backwards)) > 192


def test_fmaf_chain_is_a_true_fmaf_chain_on_every_gpu_case(chain_exe, cases):
    for name, (a, b) in cases.items():
        want, ties = probe_mod.fmaf_chain(a, b)
        assert ties == 0, name
        assert want.dtype == np.float32 and want.shape == (16, 16)
        assert np.array_equal(_bits(want), _host_chain(chain_exe, a, b)), name


def test_fmaf_chain_equals_the_headers_reference(chain_exe, cases):
    a, b = cases["normal_k64"]
    assert np.array_equal(_bits(probe_mod.fmaf_chain(a, b)[0]),
                          _host_chain(chain_exe, a, b, header=True))
    a, b = probe_mod.compute_inputs(0)["f32"]  # the quick probe's own inputs
    want, ties = probe_mod.fmaf_chain(a, b)
    assert ties == 0
    assert np.array_equal(_bits(want), _host_chain(chain_exe, a, b, header=True))
    assert np.array_equal(_bits(want), _bits(probe_mod.compute_expected_tiles(0)["f32"]))


def test_fmaf_chain_counts_ties():
    f = np.float32
    # 1 + 2^-24: half way between 1 and 1 + 2^-23; low 29 bits of the float64
    # word are 1 << 28
    acc, ties = probe_mod.fmaf_chain([[1.0, f(2.0) ** -12]], [[1.0], [f(2.0) ** -12]])
    assert ties == 1 and acc[0, 0] == 1.0
    word = np.array([1.0 + 2.0 ** -24]).view(np.uint64)[0]
    assert int(word) & ((1 << 29) - 1) == 1 << 28
    # just off the tie: no count, and the chain rounds up
    acc, ties = probe_mod.fmaf_chain([[1.0, f(2.0) ** -12]],
                                     [[1.0], [f(2.0) ** -12 * (1 + f(2.0) ** -23)]])
    assert ties == 0 and acc[0, 0] == f(1.0) + f(2.0) ** -23
    # a tie on the subnormal grid: 2^-150 is half of the smallest float32
    acc, ties = probe_mod.fmaf_chain([[f(2.0) ** -75]], [[f(2.0) ** -75]])
    assert ties == 1 and acc[0, 0] == 0.0
    acc, ties = probe_mod.fmaf_chain([[f(2.0) ** -75]], [[-(f(2.0) ** -74)]])
    assert ties == 0 and _bits(acc)[0, 0] == 0x80000001
    with pytest.raises(ValueError):
        probe_mod.fmaf_chain(np.zeros((16, 4)), np.zeros((8, 16)))


# -- bf16 rate kernel, closed form ------------------------------------------------------


def test_quick_bf16_tile_is_the_kernels_operands():
    """Thread t of a block holds a[i] = 0.5 + 0.0625 ((t + i) & 7) and b[i] =
    0.25 + 0.03125 ((3 t + i) & 7); lane l of a wave carries A[l & 31][8 (l >> 5)
    + i] and B[8 (l >> 5) + i][l & 31] (coverage.hip's operand map)."""
    a, b, d = probe_mod.quick_bf16_tile()
    assert a.shape == (32, 16) and b.shape == (16, 32) and d.shape == (32, 32)
    for t in range(256):  # all four waves of a block
        lane = t & 63
        for i in range(8):
            k = 8 * (lane >> 5) + i
            assert a[lane & 31, k] == 0.5 + 0.0625 * ((t + i) & 7)
            assert b[k, lane & 31] == 0.25 + 0.03125 * ((3 * t + i) & 7)
    # bf16 holds every operand exactly
    probe_mod.bf16_bits(a)
    probe_mod.bf16_bits(b)
    assert np.array_equal(d, np.array([[sum(a[r, k] * b[k, c] for k in range(16))
                                        for c in range(32)] for r in range(32)]))


def test_quick_bf16_sums_are_exact_in_f32_in_any_order():
    a, b, d = probe_mod.quick_bf16_tile()
    # every product is a multiple of 1/512, so every partial sum is too
    assert np.array_equal(a * 16, np.round(a * 16)) and np.array_equal(b * 32, np.round(b * 32))
    assert np.array_equal(d * 512, np.round(d * 512))
    assert not np.array_equal(d, d.T)  # a swapped row and column shows
    assert a.min() > 0 and b.min() > 0  # all terms positive: partial sums only grow
    iters = 64
    sums = probe_mod.quick_bf16_lane_sums(iters)
    assert sums.shape == (64,)
    # the largest accumulator value and the largest lane sum, in units of
    # 1/512, stay below 2^24: every intermediate is an integer float32 holds
    assert d.max() * iters * 512 < 2 ** 24
    assert sums.max() * 512 < 2 ** 24
    assert np.array_equal(sums.astype(np.float32).astype(np.float64), sums)
    # lanes differ (the data has period 8), so a lane stored in another's place shows
    assert np.unique(sums).size >= 4 and sums[0] != sums[2]
    rows = [probe_mod.quick_bf16_lane_rows(l) for l in (0, 32)]
    assert sorted(rows[0] + rows[1]) == list(range(32))
    assert rows[0][:5] == [0, 1, 2, 3, 8] and rows[1][:5] == [4, 5, 6, 7, 12]
    assert np.array_equal(probe_mod.quick_bf16_lane_sums(0), np.zeros(64))


# -- emitted code ---------------------------------------------------------------------


@pytest.fixture(scope="module")
def probe_asm(tmp_path_factory):
    """probe.hip as device assembly, with the flags the library is built with."""
    out = tmp_path_factory.mktemp("asm") / "probe.s"
    subprocess.run(
        [hip_build.HIPCC, *hip_build.DEVICE_FLAGS, "-S", "--cuda-device-only", hip_build.SRC,
         "-o", str(out)],
        check=True, capture_output=True, text=True,
    )
    functions, current = {}, None
    names = set(re.findall(r"^\s*\.type\s+([^\s,]+),@function", out.read_text(), re.M))
    for line in out.read_text().splitlines():
        label = re.match(r"^([^\s:]+):", line)
        if label and label.group(1).startswith(".Lfunc_end"):
            current = None
        elif label:
            current = label.group(1) if label.group(1) in names else current
            functions.setdefault(current, [])
        elif current is not None:
            functions[current].append(line.strip())
    return {name: body for name, body in functions.items() if name in names}


def test_build_names_the_device_flags_once():
    assert hip_build.DEVICE_FLAGS == ["--offload-arch=gfx950", "-O3"]
    assert hip_build.SRC == os.path.join(HIP_DIR, "probe.hip")


def test_rate_kernel_issues_four_independent_mfmas(probe_asm):
    """bf16_tflops credits four MFMAs per wave and iteration.  The four
    accumulators see the same operands; a compiler that merged them would
    quadruple the reported rate and no functional check could see it."""
    rate = {n: body for n, body in probe_asm.items() if "mfma_bf16_rate_kernel" in n}
    assert len(rate) == 2, sorted(probe_asm)  # the probe's and the all-lanes variant
    for name, body in rate.items():
        dests = [m.group(1) for line in body
                 for m in [re.match(r"v_mfma_f32_32x32x16_bf16\s+([av]\[\d+:\d+\])", line)] if m]
        assert len(dests) >= 4 and len(dests) % 4 == 0, (name, dests)
        assert len(set(dests)) >= 4, (name, dests)


def test_check_kernel_uses_the_f32_matrix_pipe(probe_asm):
    check = [body for n, body in probe_asm.items() if "mfma_f32_check_kernel" in n]
    assert len(check) == 1
    assert any(line.startswith("v_mfma_f32_16x16x4_f32") for line in check[0])


# -- Python plumbing ------------------------------------------------------------------


class FakeLib:
    def __init__(self, rc=0):
        self.calls = []
        self.rc = rc

    def cro_probe_run(self, device, res):
        self.calls.append(("run", device, None))
        res._obj.ok = 1
        res._obj.msg = b"ok"
        return self.rc

    def cro_probe_run_opts(self, device, opts, res):
        o = opts._obj
        self.calls.append(("run_opts", device, {n: getattr(o, n) for n, _ in o._fields_}))
        res._obj.ok = 1
        res._obj.hbm_gbps = 4321.0
        return self.rc

    def cro_probe_integrity(self, device, opts, res):
        res._obj.ok = 1
        res._obj.failed_stage = b"vram"
        return self.rc

    def cro_probe_compute(self, device, opts, res):
        res._obj.ok = 1
        res._obj.n_bad_cu_keys = 2
        res._obj.bad_cu_keys[0], res._obj.bad_cu_keys[1], res._obj.bad_cu_keys[2] = 5, 6, 7
        res._obj.reserved = 9
        res._obj.failed_test = b"lds"
        return self.rc


def test_run_probe_forwards_the_options(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(probe_mod, "_lib", fake)
    plain = probe_mod.run_probe(2)
    assert fake.calls == [("run", 2, None)]  # no options: the entry it always called
    assert plain["ok"] is True and plain["rc"] == 0 and plain["msg"] == "ok"
    got = probe_mod.run_probe(1, hbm_floor_gbps=1e9, bf16_floor_tflops=250, selftest_mode=1,
                              selftest_elem=10 * 16 + 5, selftest_bit=29)
    assert fake.calls[1] == ("run_opts", 1, {
        "hbm_floor_gbps": 1e9, "bf16_floor_tflops": 250.0, "selftest_mode": 1,
        "selftest_bit": 29, "selftest_elem": 165, "reserved": 0,
    })
    assert got["hbm_gbps"] == 4321.0
    assert set(got) == set(plain)  # the same result shape
    with pytest.raises(TypeError):
        probe_mod.run_probe(0, hbm_floor=1.0)
    fake.rc = -3
    assert probe_mod.run_probe(0, hbm_floor_gbps=1e9)["ok"] is False  # rc gates ok


QUICK_KEYS = [
    "ok", "rc", "mfma_f32_exact", "hbm_gbps", "bf16_tflops", "vram_total", "vram_free",
    "t_setup_ms", "t_mfma_ms", "t_bw_ms", "t_bf16_ms", "gcn_arch", "msg",
]
INTEGRITY_KEYS = [
    "ok", "rc", "n_bad", "first_bad_byte", "bits_bad", "vram_passes", "link_passes",
    "vram_chunks", "vram_bytes_verified", "h2d_dma_bytes_verified", "d2h_dma_bytes_verified",
    "h2d_kernel_bytes_verified", "d2h_kernel_bytes_verified", "vram_n_bad", "h2d_dma_n_bad",
    "d2h_dma_n_bad", "h2d_kernel_n_bad", "d2h_kernel_n_bad", "vram_fill_gbps",
    "vram_verify_gbps", "h2d_dma_gbps", "d2h_dma_gbps", "h2d_kernel_gbps", "d2h_kernel_gbps",
    "t_vram_ms", "t_link_dma_ms", "t_link_kernel_ms", "t_total_ms", "failed_stage", "msg",
    "first_bad_got",
]
COMPUTE_KEYS = [
    "ok", "rc", "cus_expected", "rounds", "waves_run", "waves_bad", "bad_f32", "bad_i8",
    "bad_bf16", "bad_lds", "first_bad_index", "cus_seen", "xcds_seen", "simds_seen", "cus_bad",
    "xcd", "se", "sh", "cu", "simd", "first_fail_mask", "n_bad", "first_bad", "bits_bad",
    "n_bad_cu_keys", "bad_cu_keys", "first_bad_round", "first_bad_record", "grid_blocks",
    "lds_bytes", "iters", "gpu_ms", "t_total_ms", "failed_test", "msg",
]


def test_result_dicts_keep_their_keys_order_and_types(monkeypatch):
    """What run_probe, run_integrity and run_compute hand to the controller and
    what croagent prints share these shapes: the keys in this order, booleans
    where the struct holds a flag, text decoded, and of the compute result's
    eight key slots only the ones in use."""
    monkeypatch.setattr(probe_mod, "_lib", FakeLib(rc=-7))
    quick = probe_mod.run_probe(0)
    integrity = probe_mod.run_integrity(0)
    compute = probe_mod.run_compute(0)
    assert list(quick) == QUICK_KEYS
    assert list(integrity) == INTEGRITY_KEYS
    assert list(compute) == COMPUTE_KEYS  # no "reserved"
    for got in (quick, integrity, compute):
        assert got["ok"] is False and got["rc"] == -7  # ok in the struct, but rc gates it
        assert isinstance(got["msg"], str)
        for key, value in got.items():
            assert not isinstance(value, bytes), key
    assert quick["mfma_f32_exact"] is False and quick["msg"] == "ok" and quick["gcn_arch"] == ""
    assert type(quick["hbm_gbps"]) is float and type(quick["vram_total"]) is int
    assert integrity["failed_stage"] == "vram" and type(integrity["n_bad"]) is int
    assert compute["bad_cu_keys"] == [5, 6] and compute["n_bad_cu_keys"] == 2
    assert all(type(k) is int for k in compute["bad_cu_keys"])
    assert compute["failed_test"] == "lds" and type(compute["gpu_ms"]) is float


def test_probe_hooks_untouched(monkeypatch):
    assert probe_mod.make_probe_fn("quick") is probe_mod.probe_fn_for_nodeops
    fake = FakeLib()
    monkeypatch.setattr(probe_mod, "_lib", fake)
    monkeypatch.setattr(probe_mod, "hip_device_for_bdf", lambda bdf: 3)

    class Gpu:
        pci_bdf = "0000:05:00.0"

    assert probe_mod.probe_fn_for_nodeops(Gpu())["ok"] is True
    assert fake.calls == [("run", 3, None)]

    class Exec:
        argv = None

        def run(self, node, argv, timeout=None):
            Exec.argv = list(argv)
            return 0, '{"ok": true}', ""

    assert probe_mod.make_exec_probe_fn(Exec(), "n0")(Gpu()) == {"ok": True}
    assert Exec.argv == ["croagent", "probe", "--bdf", "0000:05:00.0"]
