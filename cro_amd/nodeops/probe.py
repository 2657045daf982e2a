"""ctypes wrapper for the gfx950 health probe (cro_amd/hip/probe.hip).

Fails LOUDLY when running on a GPU node without the compiled extension —
a silent fallback would let GPU tests pass without the native path
(the operator must never advertise a device it could not verify).
"""

from __future__ import annotations

import ctypes
import os
from typing import Optional

_LIB_PATH = os.path.join(os.path.dirname(__file__), "..", "hip", "libcroprobe.so")


class CroProbeResult(ctypes.Structure):
    _fields_ = [
        ("ok", ctypes.c_int),
        ("mfma_f32_exact", ctypes.c_int),
        ("hbm_gbps", ctypes.c_double),
        ("bf16_tflops", ctypes.c_double),
        ("vram_total", ctypes.c_longlong),
        ("vram_free", ctypes.c_longlong),
        ("t_setup_ms", ctypes.c_double),
        ("t_mfma_ms", ctypes.c_double),
        ("t_bw_ms", ctypes.c_double),
        ("t_bf16_ms", ctypes.c_double),
        ("gcn_arch", ctypes.c_char * 64),
        ("msg", ctypes.c_char * 256),
    ]


class CroProbeOpts(ctypes.Structure):
    """Mirror of ``struct CroProbeOpts`` (cro_amd/hip/croprobe.h)."""

    _fields_ = [
        ("hbm_floor_gbps", ctypes.c_double),
        ("bf16_floor_tflops", ctypes.c_double),
        ("selftest_mode", ctypes.c_int),
        ("selftest_bit", ctypes.c_int),
        ("selftest_elem", ctypes.c_uint),
        ("reserved", ctypes.c_int),
    ]


class CroProbeWindows(ctypes.Structure):
    """Mirror of ``struct CroProbeWindows`` (cro_amd/hip/croprobe.h)."""

    _fields_ = [
        ("copy_launches", ctypes.c_int),
        ("bf16_iters", ctypes.c_int),
        ("skip_check_launch", ctypes.c_int),
        ("reserved", ctypes.c_int),
    ]


class CroIntegrityOpts(ctypes.Structure):
    """Mirror of ``struct CroIntegrityOpts`` (cro_amd/hip/croprobe.h)."""

    _fields_ = [
        ("vram_bytes", ctypes.c_longlong),
        ("link_bytes", ctypes.c_longlong),
        ("chunk_bytes", ctypes.c_longlong),
        ("seed", ctypes.c_uint),
        ("selftest_stage", ctypes.c_int),
        ("link_floor_gbps", ctypes.c_double),
        ("selftest_pass", ctypes.c_int),
        ("selftest_bit", ctypes.c_int),
        ("selftest_word", ctypes.c_ulonglong),
    ]


INTEGRITY_STAGES = ("vram", "h2d_dma", "d2h_dma", "h2d_kernel", "d2h_kernel")
INTEGRITY_RATES = (
    "vram_fill_gbps",
    "vram_verify_gbps",
    "h2d_dma_gbps",
    "d2h_dma_gbps",
    "h2d_kernel_gbps",
    "d2h_kernel_gbps",
)


class CroIntegrityResult(ctypes.Structure):
    """Mirror of ``struct CroIntegrityResult`` (cro_amd/hip/croprobe.h)."""

    _fields_ = (
        [
            ("ok", ctypes.c_int),
            ("rc", ctypes.c_int),
            ("n_bad", ctypes.c_ulonglong),
            ("first_bad_byte", ctypes.c_ulonglong),
            ("bits_bad", ctypes.c_uint),
            ("vram_passes", ctypes.c_int),
            ("link_passes", ctypes.c_int),
            ("vram_chunks", ctypes.c_int),
        ]
        + [(f"{s}_bytes_verified", ctypes.c_longlong) for s in INTEGRITY_STAGES]
        + [(f"{s}_n_bad", ctypes.c_ulonglong) for s in INTEGRITY_STAGES]
        + [(r, ctypes.c_double) for r in INTEGRITY_RATES]
        + [
            ("t_vram_ms", ctypes.c_double),
            ("t_link_dma_ms", ctypes.c_double),
            ("t_link_kernel_ms", ctypes.c_double),
            ("t_total_ms", ctypes.c_double),
            ("failed_stage", ctypes.c_char * 32),
            ("msg", ctypes.c_char * 256),
            ("first_bad_got", ctypes.c_uint),
            ("reserved", ctypes.c_int),
        ]
    )


class CroComputeOpts(ctypes.Structure):
    """Mirror of ``struct CroComputeOpts`` (cro_amd/hip/croprobe.h)."""

    _fields_ = [
        ("grid_blocks", ctypes.c_int),
        ("lds_bytes", ctypes.c_int),
        ("iters", ctypes.c_int),
        ("max_rounds", ctypes.c_int),
        ("seed", ctypes.c_uint),
        ("selftest_mode", ctypes.c_int),
        ("selftest_test", ctypes.c_int),
        ("selftest_bit", ctypes.c_int),
        ("selftest_elem", ctypes.c_uint),
        ("selftest_key", ctypes.c_uint),
        ("selftest_span", ctypes.c_uint),
        ("selftest_pass", ctypes.c_int),
        ("min_cu_fraction", ctypes.c_double),
    ]


class CroCoverageRecord(ctypes.Structure):
    """Mirror of ``struct CroCoverageRecord`` (cro_amd/hip/crocoverage.h)."""

    _fields_ = [
        ("xcc_id", ctypes.c_uint),
        ("hw_id", ctypes.c_uint),
        ("fail_mask", ctypes.c_uint),
        ("n_bad", ctypes.c_uint),
        ("first_bad", ctypes.c_uint),
        ("bits_bad", ctypes.c_uint),
        ("valid", ctypes.c_uint),
        ("reserved", ctypes.c_uint),
    ]


COMPUTE_TESTS = ("mfma_f32", "mfma_i8", "mfma_bf16", "lds")
# fields of the nested ``struct CroCoverageAgg`` (crocoverage.h), in order
COMPUTE_AGG_FIELDS = (
    [(n, ctypes.c_ulonglong) for n in
     ("waves_run", "waves_bad", "bad_f32", "bad_i8", "bad_bf16", "bad_lds")]
    + [("first_bad_index", ctypes.c_longlong)]
    + [(n, ctypes.c_int) for n in
       ("cus_seen", "xcds_seen", "simds_seen", "cus_bad", "xcd", "se", "sh", "cu", "simd")]
    + [(n, ctypes.c_uint) for n in ("first_fail_mask", "n_bad", "first_bad", "bits_bad")]
    + [("n_bad_cu_keys", ctypes.c_int), ("bad_cu_keys", ctypes.c_uint * 8)]
)


class CroComputeResult(ctypes.Structure):
    """Mirror of ``struct CroComputeResult`` (cro_amd/hip/croprobe.h), with
    the nested aggregate's fields written out flat."""

    _fields_ = (
        [
            ("ok", ctypes.c_int),
            ("rc", ctypes.c_int),
            ("cus_expected", ctypes.c_int),
            ("rounds", ctypes.c_int),
        ]
        + COMPUTE_AGG_FIELDS
        + [
            ("first_bad_round", ctypes.c_int),
            ("first_bad_record", ctypes.c_int),
            ("grid_blocks", ctypes.c_int),
            ("lds_bytes", ctypes.c_int),
            ("iters", ctypes.c_int),
            ("reserved", ctypes.c_int),
            ("gpu_ms", ctypes.c_double),
            ("t_total_ms", ctypes.c_double),
            ("failed_test", ctypes.c_char * 16),
            ("msg", ctypes.c_char * 256),
        ]
    )


PROBE_LEVELS = ("quick", "deep")

_lib = None


def _gpu_present() -> bool:
    return os.path.exists("/dev/kfd")


def load_library(required: Optional[bool] = None) -> Optional[ctypes.CDLL]:
    """Load libcroprobe.so.  required=None → required iff a GPU is present."""
    global _lib
    if _lib is not None:
        return _lib
    if required is None:
        required = _gpu_present()
    path = os.path.abspath(_LIB_PATH)
    if not os.path.exists(path):
        if required:
            raise RuntimeError(
                f"libcroprobe.so missing at {path} on a GPU node — build it with "
                "`python -m cro_amd.hip.build` (hipcc --offload-arch=gfx950)"
            )
        return None
    lib = ctypes.CDLL(path)
    lib.cro_probe_run.argtypes = [ctypes.c_int, ctypes.POINTER(CroProbeResult)]
    lib.cro_probe_run.restype = ctypes.c_int
    lib.cro_probe_run_opts.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroProbeOpts), ctypes.POINTER(CroProbeResult),
    ]
    lib.cro_probe_run_opts.restype = ctypes.c_int
    lib.cro_probe_run_windows.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroProbeWindows), ctypes.POINTER(CroProbeResult),
    ]
    lib.cro_probe_run_windows.restype = ctypes.c_int
    f32p = ctypes.POINTER(ctypes.c_float)
    lib.cro_probe_mfma_f32.argtypes = [ctypes.c_int, f32p, f32p, f32p, ctypes.c_int]
    lib.cro_probe_mfma_f32.restype = ctypes.c_int
    lib.cro_probe_copy.argtypes = [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_void_p,
        ctypes.POINTER(ctypes.c_int),
    ]
    lib.cro_probe_copy.restype = ctypes.c_int
    lib.cro_probe_bw_selfcheck.argtypes = [
        ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong),
    ]
    lib.cro_probe_bw_selfcheck.restype = ctypes.c_int
    lib.cro_probe_bf16_sink.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
    ]
    lib.cro_probe_bf16_sink.restype = ctypes.c_int
    lib.cro_probe_device_count.restype = ctypes.c_int
    lib.cro_probe_pci_bus_id.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    lib.cro_probe_pci_bus_id.restype = ctypes.c_int
    lib.cro_probe_alloc.argtypes = [ctypes.c_int, ctypes.c_longlong]
    lib.cro_probe_alloc.restype = ctypes.c_void_p
    lib.cro_probe_free.argtypes = [ctypes.c_void_p]
    lib.cro_probe_free.restype = None
    lib.cro_probe_integrity.argtypes = [
        ctypes.c_int,
        ctypes.POINTER(CroIntegrityOpts),
        ctypes.POINTER(CroIntegrityResult),
    ]
    lib.cro_probe_integrity.restype = ctypes.c_int
    u32p = ctypes.POINTER(ctypes.c_uint)
    u64p = ctypes.POINTER(ctypes.c_ulonglong)
    lib.cro_probe_pattern_fill.argtypes = [
        ctypes.c_int, ctypes.c_uint, ctypes.c_int,
        ctypes.c_ulonglong, ctypes.c_ulonglong, u32p, ctypes.POINTER(ctypes.c_int),
    ]
    lib.cro_probe_pattern_fill.restype = ctypes.c_int
    lib.cro_probe_pattern_verify.argtypes = [
        ctypes.c_int, ctypes.c_uint, ctypes.c_int,
        ctypes.c_ulonglong, ctypes.c_ulonglong, u32p, u64p, u64p, u32p,
    ]
    lib.cro_probe_pattern_verify.restype = ctypes.c_int
    lib.cro_probe_compute.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroComputeOpts), ctypes.POINTER(CroComputeResult),
    ]
    lib.cro_probe_compute.restype = ctypes.c_int
    lib.cro_probe_compute_records.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroComputeOpts), ctypes.POINTER(CroComputeResult),
        ctypes.POINTER(CroCoverageRecord), ctypes.c_int,
    ]
    lib.cro_probe_compute_records.restype = ctypes.c_int
    lib.cro_probe_compute_tiles.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroComputeOpts), ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.POINTER(CroComputeResult), ctypes.POINTER(CroCoverageRecord),
        ctypes.c_int,
    ]
    lib.cro_probe_compute_tiles.restype = ctypes.c_int
    lib.cro_probe_compute_lds_dump.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_int,
        ctypes.c_uint, ctypes.c_uint, ctypes.c_int, ctypes.c_void_p, u32p,
    ]
    lib.cro_probe_compute_lds_dump.restype = ctypes.c_int
    lib.cro_probe_mfma_tile.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_int,
    ]
    lib.cro_probe_mfma_tile.restype = ctypes.c_int
    _lib = lib
    return lib


def vram_alloc(device: int, nbytes: int):
    """Allocate+touch VRAM on a device; returns an opaque handle (None on
    failure).  Used by the self-pid fingerprint."""
    lib = load_library(required=True)
    return lib.cro_probe_alloc(device, nbytes)


def vram_free(handle) -> None:
    if handle:
        load_library(required=True).cro_probe_free(handle)


def device_count() -> int:
    lib = load_library()
    if lib is None:
        return 0
    return max(lib.cro_probe_device_count(), 0)


_bdf_cache = {}


def hip_device_for_bdf(pci_bdf: str) -> Optional[int]:
    """Map a PCI DBDF (from KFD topology) to a HIP device ordinal (cached —
    hipDeviceGetPCIBusId is sysfs-backed and the probe runs per attach)."""
    want = pci_bdf.lower()
    if want in _bdf_cache:
        return _bdf_cache[want]
    lib = load_library()
    if lib is None:
        return None
    buf = ctypes.create_string_buffer(64)
    for dev in range(device_count()):
        if lib.cro_probe_pci_bus_id(dev, buf, 64) == 0:
            if buf.value.decode().lower().startswith(want.rsplit(".", 1)[0]):
                _bdf_cache[want] = dev
                return dev
    return None


def _probe_opts(hbm_floor_gbps=0.0, bf16_floor_tflops=0.0, selftest_mode=0, selftest_bit=0,
                selftest_elem=0) -> "CroProbeOpts":
    return CroProbeOpts(
        hbm_floor_gbps=float(hbm_floor_gbps), bf16_floor_tflops=float(bf16_floor_tflops),
        selftest_mode=int(selftest_mode), selftest_bit=int(selftest_bit),
        selftest_elem=int(selftest_elem) & 0xFFFFFFFF,
    )


def _result_dict(res: ctypes.Structure, rc: int) -> dict:
    """A result struct as the dict the controller and the tests see: ``ok``
    (gated by rc) and ``rc`` first, then the struct's other fields in order;
    text decoded, flags as bool, of the bad-CU key slots only those in use,
    and ``reserved`` dropped."""
    out = {"ok": bool(res.ok) and rc == 0, "rc": rc}
    for name, _ in res._fields_:
        if name in ("ok", "rc", "reserved"):
            continue
        value = getattr(res, name)
        if name == "mfma_f32_exact":
            value = bool(value)
        elif name == "bad_cu_keys":
            value = [int(k) for k in value][: res.n_bad_cu_keys]
        elif isinstance(value, bytes):
            value = value.decode(errors="replace")
        out[name] = value
    return out


def run_probe(device: int = 0, **opts) -> dict:
    """Quick probe.  Options as ``struct CroProbeOpts``; zero takes the library
    default (floors of 500 GB/s and 100 TF).  The ``selftest_*`` options are
    for tests.  Without options this is ``cro_probe_run``, as ever."""
    lib = load_library(required=True)
    res = CroProbeResult()
    if opts:
        c_opts = _probe_opts(**opts)
        rc = lib.cro_probe_run_opts(device, ctypes.byref(c_opts), ctypes.byref(res))
    else:
        rc = lib.cro_probe_run(device, ctypes.byref(res))
    return _result_dict(res, rc)


def run_probe_windows(device: int = 0, copy_launches: int = 0, bf16_iters: int = 0,
                      skip_check_launch: int = 0) -> dict:
    """The quick probe's pipeline at the caller's rate windows (``struct
    CroProbeWindows``; zero takes the library default, which is what
    ``run_probe`` runs at), with the floors at their defaults.
    ``skip_check_launch`` is for tests: the check kernel is left out, so the
    exact gate must fail on the poisoned tile."""
    lib = load_library(required=True)
    windows = CroProbeWindows(
        copy_launches=int(copy_launches), bf16_iters=int(bf16_iters),
        skip_check_launch=int(skip_check_launch),
    )
    res = CroProbeResult()
    rc = lib.cro_probe_run_windows(device, ctypes.byref(windows), ctypes.byref(res))
    return _result_dict(res, rc)


def probe_fn_for_nodeops(gpu) -> dict:
    """AmdNodeOps probe hook: GPUDevice → probe result on the right ordinal."""
    dev = hip_device_for_bdf(gpu.pci_bdf)
    if dev is None:
        dev = 0
    return run_probe(dev)


# -- quick probe: raw kernel entries and their references, for tests ---------------


def mfma_f32_tile(device: int, a, b):
    """One wave of the quick probe's f32 check kernel on caller data:
    16xK @ Kx16 → float32 16x16, K a multiple of 4, at most 4096."""
    import numpy as np

    lib = load_library(required=True)
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    k = a.shape[1] if a.ndim == 2 else -1
    if a.shape != (16, k) or b.shape != (k, 16):
        raise ValueError("f32 tile wants A 16xK and B Kx16")
    d = np.zeros((16, 16), dtype=np.float32)
    f32p = ctypes.POINTER(ctypes.c_float)
    rc = lib.cro_probe_mfma_f32(device, a.ctypes.data_as(f32p), b.ctypes.data_as(f32p),
                                d.ctypes.data_as(f32p), k)
    if rc != 0:
        raise RuntimeError(f"cro_probe_mfma_f32 failed: rc={rc}")
    return d


def copy_vectors(device: int, words, grid_blocks: int) -> dict:
    """Run the quick probe's copy kernel over ``words`` (uint32, four per
    16-byte vector) with ``grid_blocks`` x 256 threads.  Returns the copy, and
    whether the 64 guard vectors after it and the source came back untouched."""
    import numpy as np

    lib = load_library(required=True)
    src = np.ascontiguousarray(words, dtype=np.uint32)
    if src.ndim != 1 or src.size % 4:
        raise ValueError("copy_vectors wants a flat array of whole 16-byte vectors")
    dst = np.zeros_like(src)
    guard_ok = ctypes.c_int(0)
    rc = lib.cro_probe_copy(device, src.ctypes.data, src.size // 4, int(grid_blocks),
                            dst.ctypes.data, ctypes.byref(guard_ok))
    if rc not in (0, -11):
        raise RuntimeError(f"cro_probe_copy failed: rc={rc}")
    return {"dst": dst, "guard_ok": bool(guard_ok.value), "src_unchanged": rc == 0}


def bw_selfcheck(device: int = 0) -> dict:
    """The quick probe's own copy launch, once, into a zeroed ``dst``: how many
    of the bytes it is credited for did not arrive."""
    lib = load_library(required=True)
    n_bad = ctypes.c_ulonglong()
    first_bad = ctypes.c_ulonglong()
    rc = lib.cro_probe_bw_selfcheck(device, ctypes.byref(n_bad), ctypes.byref(first_bad))
    if rc != 0:
        raise RuntimeError(f"cro_probe_bw_selfcheck failed: rc={rc}")
    return {"n_bad": n_bad.value, "first_bad": first_bad.value}


def bf16_sink(device: int, blocks: int, iters: int, all_lanes: bool):
    """What the quick probe's bf16 rate kernel stores: thread 0's sum of each
    block, or with ``all_lanes`` every thread's (blocks * 256 values)."""
    import numpy as np

    lib = load_library(required=True)
    n = max(int(blocks), 0) * (256 if all_lanes else 1)
    out = np.zeros(n, dtype=np.float32)
    rc = lib.cro_probe_bf16_sink(device, int(blocks), int(iters), 1 if all_lanes else 0,
                                 out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"cro_probe_bf16_sink failed: rc={rc}")
    return out


def fmaf_chain(a, b):
    """The k-ordered float32 fused-multiply-add chain of ``a`` (MxK) @ ``b``
    (KxN), which the f32 matrix pipe of gfx950 equals bit for bit, and the
    number of steps at which this numpy form could differ from a true ``fmaf``.

    The product of two float32 is exact in float64; the sum with the
    accumulator is rounded once to float64 and then to float32.  That double
    rounding differs from the single one of ``fmaf`` only when the float64 sum
    lies exactly half way between two neighbouring float32 values — for a
    normal result: the low 29 bits of the float64 word are ``1 << 28``.  Such
    steps are counted (for subnormal results too, where the float32 grid is
    coarser); at a count of 0 the result is the true chain."""
    import numpy as np

    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[0]:
        raise ValueError("fmaf_chain wants A MxK and B KxN")
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    ties = 0
    for k in range(a.shape[1]):
        prod = a[:, k : k + 1].astype(np.float64) * b[k : k + 1, :].astype(np.float64)
        total = prod + acc.astype(np.float64)
        acc = total.astype(np.float32)
        # both differences are exact: a tie is half the way to the neighbour
        # of the rounded value on the side of the float64 sum
        off = total - acc.astype(np.float64)
        toward = np.where(off > 0, np.float32(np.inf), np.float32(-np.inf))
        gap = np.nextafter(acc, toward).astype(np.float64) - acc.astype(np.float64)
        with np.errstate(invalid="ignore"):
            ties += int(np.count_nonzero((off != 0) & (2.0 * off == gap)))
    return acc, ties


def quick_bf16_tile():
    """Closed form of the quick probe's bf16 rate kernel: the operands every
    wave holds, A 32x16 and B 16x32, and D = A @ B (float64, exact)."""
    import numpy as np

    row, k = np.meshgrid(np.arange(32), np.arange(16), indexing="ij")
    a = 0.5 + 0.0625 * ((row + k) & 7)
    kk, col = np.meshgrid(np.arange(16), np.arange(32), indexing="ij")
    b = 0.25 + 0.03125 * ((3 * col + kk) & 7)
    return a, b, a @ b


def quick_bf16_lane_rows(lane: int):
    """Rows of the 32x32 tile that lane ``lane`` of a wave accumulates (of
    column ``lane & 31``): register r is row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)."""
    return [(r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) for r in range(16)]


def quick_bf16_lane_sums(iters: int):
    """What each of a wave's 64 lanes sums up in the rate kernel after ``iters``
    iterations of its four accumulators (float64)."""
    import numpy as np

    d = quick_bf16_tile()[2]
    return np.array([4.0 * iters * d[quick_bf16_lane_rows(l), l & 31].sum() for l in range(64)])


def run_integrity(
    device: int = 0,
    vram_bytes: int = 0,
    link_bytes: int = 0,
    seed: int = 0,
    link_floor_gbps: float = 0.0,
    chunk_bytes: int = 0,
    selftest_stage=0,
    selftest_pass: int = 0,
    selftest_bit: int = 0,
    selftest_word: int = 0,
) -> dict:
    """Deep probe: verify the content of ``vram_bytes`` of VRAM and of
    ``link_bytes`` moved across the host link in both directions, by copy
    engine and by shader (cro_amd/hip/integrity.hip).  Zero sizes take the
    library defaults.  Gates on data only, unless ``link_floor_gbps`` > 0.

    The ``selftest_*`` options are for tests: in ``selftest_stage`` (a name of
    ``INTEGRITY_STAGES`` or its number, 1-based; 0 is off) the host flips bit
    ``selftest_bit`` of word ``selftest_word`` of the stage's span between the
    write and the compare, for VRAM in pass ``selftest_pass``."""
    lib = load_library(required=True)
    if isinstance(selftest_stage, str):
        selftest_stage = INTEGRITY_STAGES.index(selftest_stage) + 1
    opts = CroIntegrityOpts(
        vram_bytes=int(vram_bytes),
        link_bytes=int(link_bytes),
        chunk_bytes=int(chunk_bytes),
        seed=int(seed) & 0xFFFFFFFF,
        link_floor_gbps=float(link_floor_gbps),
        selftest_stage=int(selftest_stage),
        selftest_pass=int(selftest_pass),
        selftest_bit=int(selftest_bit),
        selftest_word=int(selftest_word),
    )
    res = CroIntegrityResult()
    rc = lib.cro_probe_integrity(device, ctypes.byref(opts), ctypes.byref(res))
    return _result_dict(res, rc)


def pattern_words(base_word: int, n_words: int, seed: int, invert):
    """numpy reference of the deep probe's pattern (cro_amd/hip/cropattern.h):
    the uint32 words at global word indices base_word .. base_word+n_words."""
    import numpy as np

    w = np.uint64(base_word) + np.arange(n_words, dtype=np.uint64)
    x = (w & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ np.uint32(seed & 0xFFFFFFFF)
    x = x + (w >> np.uint64(32)).astype(np.uint32) * np.uint32(0x9E3779B9)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return ~x if invert else x


def pattern_fill(device: int, seed: int, invert, base_word: int, n_words: int):
    """Run the fill kernel on ``n_words`` of VRAM and return them (uint32).
    Raises when the kernel wrote anything after word ``n_words`` (the slack of
    the last vector and a guard band are preset and read back)."""
    import numpy as np

    lib = load_library(required=True)
    out = np.zeros(n_words, dtype=np.uint32)
    guard_ok = ctypes.c_int(0)
    rc = lib.cro_probe_pattern_fill(
        device, seed & 0xFFFFFFFF, 1 if invert else 0, base_word, n_words,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), ctypes.byref(guard_ok),
    )
    if rc != 0:
        raise RuntimeError(f"cro_probe_pattern_fill failed: rc={rc}")
    if not guard_ok.value:
        raise RuntimeError(f"cro_probe_pattern_fill wrote past its {n_words} words")
    return out


def pattern_verify(device: int, seed: int, invert, base_word: int, words) -> dict:
    """Upload ``words`` (uint32 array) and run the verify kernel on them."""
    import numpy as np

    lib = load_library(required=True)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    n_bad = ctypes.c_ulonglong()
    first_bad = ctypes.c_ulonglong()
    bits_bad = ctypes.c_uint()
    rc = lib.cro_probe_pattern_verify(
        device, seed & 0xFFFFFFFF, 1 if invert else 0, base_word, words.size,
        words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)),
        ctypes.byref(n_bad), ctypes.byref(first_bad), ctypes.byref(bits_bad),
    )
    if rc != 0:
        raise RuntimeError(f"cro_probe_pattern_verify failed: rc={rc}")
    return {"n_bad": n_bad.value, "first_bad": first_bad.value, "bits_bad": bits_bad.value}


# -- compute-coverage stage (cro_amd/hip/coverage.hip) ----------------------------


def _compute_opts(grid_blocks=0, lds_bytes=0, iters=0, max_rounds=0, seed=0,
                  min_cu_fraction=0.0, selftest_mode=0, selftest_test=0, selftest_elem=0,
                  selftest_bit=0, selftest_key=0, selftest_span=0,
                  selftest_pass=0) -> "CroComputeOpts":
    if isinstance(selftest_test, str):
        selftest_test = COMPUTE_TESTS.index(selftest_test)
    return CroComputeOpts(
        grid_blocks=int(grid_blocks), lds_bytes=int(lds_bytes), iters=int(iters),
        max_rounds=int(max_rounds), seed=int(seed) & 0xFFFFFFFF,
        selftest_mode=int(selftest_mode), selftest_test=int(selftest_test),
        selftest_bit=int(selftest_bit), selftest_elem=int(selftest_elem),
        selftest_key=int(selftest_key), selftest_span=int(selftest_span),
        selftest_pass=int(selftest_pass), min_cu_fraction=float(min_cu_fraction),
    )


# expected tiles a caller may hand to run_compute_records: name, dtype, elements
COMPUTE_TILE_SPECS = (("f32", "float32", 256), ("i8", "int32", 256), ("bf16", "float32", 1024))


def _caller_tiles(tiles) -> list:
    """The three tile arguments of cro_probe_compute_tiles, in the C order:
    a contiguous array of the tile's own type and size, or None."""
    import numpy as np

    tiles = dict(tiles or {})
    out = []
    for name, dtype, elems in COMPUTE_TILE_SPECS:
        tile = tiles.pop(name, None)
        if tile is not None:
            tile = np.asarray(tile)
            if tile.dtype != np.dtype(dtype) or tile.size != elems:
                raise ValueError(f"{name} tile wants {elems} values of {dtype}")
            tile = np.ascontiguousarray(tile).reshape(-1)
        out.append(tile)
    if tiles:
        raise ValueError(f"unknown tiles: {sorted(tiles)}")
    return out


def run_compute(device: int = 0, **opts) -> dict:
    """Compute-coverage stage: exact f32, i8 and bf16 matrix checks and an LDS
    march on every CU and SIMD, with the location of the first bad wave
    (cro_amd/hip/coverage.hip).  Options as ``struct CroComputeOpts``; zero
    takes the library default.  A data mismatch always fails; coverage is
    reported and gates only when ``min_cu_fraction`` > 0.  The ``selftest_*``
    options are for tests."""
    lib = load_library(required=True)
    c_opts = _compute_opts(**opts)
    res = CroComputeResult()
    rc = lib.cro_probe_compute(device, ctypes.byref(c_opts), ctypes.byref(res))
    return _result_dict(res, rc)


def _run_with_records(record_type, c_opts, res, call):
    """What the per-wave stages' run_*_records share: a buffer of
    ``record_type`` sized for the options, ``call(buf, cap)`` (the library's
    *_records entry; returns its rc), and the records it returned as a
    structured numpy array next to the result dict."""
    import numpy as np

    # room for what was asked; a default grid is one workgroup per CU, and
    # no device of this family has more than 1024 of them
    blocks = c_opts.grid_blocks or 1024
    rounds = c_opts.max_rounds or 4
    cap = max(blocks * 4 * rounds, 1)
    buf = (record_type * cap)()
    out = _result_dict(res, call(buf, cap))
    n = min(out["rounds"] * out["grid_blocks"] * 4, cap)
    dtype = np.dtype([(name, np.uint32) for name, _ in record_type._fields_])
    return out, np.frombuffer(buf, dtype=dtype, count=cap)[:n].copy()


def run_compute_records(device: int = 0, tiles=None, **opts):
    """As run_compute, and returns the raw per-wave records as well: a
    structured numpy array of rounds * grid_blocks * 4 records, round-major.
    ``tiles`` (for tests): a dict with any of ``"f32"`` (256 float32), ``"i8"``
    (256 int32) and ``"bf16"`` (1024 float32), each taking the place of that
    test's expected tile in this call only."""
    lib = load_library(required=True)
    c_opts = _compute_opts(**opts)
    c_tiles = _caller_tiles(tiles)
    res = CroComputeResult()
    return _run_with_records(CroCoverageRecord, c_opts, res, lambda buf, cap: (
        lib.cro_probe_compute_tiles(
            device, ctypes.byref(c_opts),
            *[t.ctypes.data if t is not None else None for t in c_tiles],
            ctypes.byref(res), buf, cap)))


def compute_lds_dump(device: int, grid_blocks: int, lds_bytes: int, seed: int = 0, invert=0,
                     plant_elem: int = 0, plant_span: int = 0, plant_bit: int = 0):
    """What the coverage kernel's march wrote (for tests): each workgroup's LDS
    after the fill of the pattern (``invert`` 0) or complement pass and, with
    ``plant_span`` > 0, a plant as self-test mode 3 makes it.  Returns a uint32
    array of grid_blocks x lds_bytes / 4 words and how many guard words after
    the marched ones changed (always 0 where the size leaves no room for a
    guard, above 163840 - 1024 bytes)."""
    import numpy as np

    lib = load_library(required=True)
    words = np.zeros((max(int(grid_blocks), 0), max(int(lds_bytes), 0) // 4), dtype=np.uint32)
    guard_bad = ctypes.c_uint(0)
    rc = lib.cro_probe_compute_lds_dump(
        device, int(grid_blocks), int(lds_bytes), int(seed) & 0xFFFFFFFF, 1 if invert else 0,
        int(plant_elem), int(plant_span), int(plant_bit), words.ctypes.data,
        ctypes.byref(guard_bad),
    )
    if rc != 0:
        raise RuntimeError(f"cro_probe_compute_lds_dump failed: rc={rc}")
    return words, guard_bad.value


def lds_verify_wave(word):
    """The wave of a workgroup that verifies LDS word ``word`` in the coverage
    kernel's march: 16-byte vector v = word // 4 is checked by thread v % 256,
    that is wave (v // 64) % 4.  int or numpy array."""
    return ((word // 4) // 64) % 4


def lds_plant_per_wave(elem: int, span: int):
    """For a plant of ``span`` words from ``elem`` on: per wave 0..3 how many of
    them it verifies and the lowest (0xFFFFFFFF where it verifies none)."""
    import numpy as np

    words = np.arange(elem, elem + span, dtype=np.int64)
    owner = lds_verify_wave(words)
    counts = [int((owner == w).sum()) for w in range(4)]
    firsts = [int(words[owner == w].min()) if counts[w] else 0xFFFFFFFF for w in range(4)]
    return counts, firsts


MFMA_TILE_KINDS = {"i8": 1, "bf16": 2}


def bf16_bits(values):
    """bf16 bit patterns (uint16) of float32 values that bf16 holds exactly."""
    import numpy as np

    u = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)
    if np.any(u & np.uint32(0xFFFF)):
        raise ValueError("value not exactly representable in bf16")
    return (u >> np.uint32(16)).astype(np.uint16)


def mfma_tile(device: int, kind: str, a, b):
    """One wave of the coverage kernel's i8 (16xK @ Kx16 → int32 16x16) or
    bf16 (32xK @ Kx32 → float32 32x32; inputs given as numbers bf16 holds
    exactly) matrix product on caller data."""
    import numpy as np

    lib = load_library(required=True)
    rows = 16 if kind == "i8" else 32
    a = np.asarray(a)
    b = np.asarray(b)
    k = a.shape[1]
    if a.shape != (rows, k) or b.shape != (k, rows):
        raise ValueError(f"{kind} tile wants A {rows}xK and B Kx{rows}")
    if kind == "i8":
        a_dev = np.ascontiguousarray(a, dtype=np.int8)
        b_dev = np.ascontiguousarray(b, dtype=np.int8)
        d = np.zeros((rows, rows), dtype=np.int32)
    else:
        a_dev, b_dev = bf16_bits(a), bf16_bits(b)
        d = np.zeros((rows, rows), dtype=np.float32)
    rc = lib.cro_probe_mfma_tile(
        device, MFMA_TILE_KINDS[kind], a_dev.ctypes.data, b_dev.ctypes.data, d.ctypes.data, k
    )
    if rc != 0:
        raise RuntimeError(f"cro_probe_mfma_tile failed: rc={rc}")
    return d


def _lcg_stream(state: int, n: int):
    """n steps of the probe's LCG (probe.hip, crocoverage.h) from ``state``."""
    import numpy as np

    out = np.empty(n, dtype=np.uint32)
    for i in range(n):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = state
    return out, state


def compute_inputs(seed: int = 0) -> dict:
    """numpy mirror of the compute stage's inputs (crocoverage.h): f32
    A 16x64 / B 64x16, i8 A 16x256 / B 256x16, bf16 A 32x64 / B 64x32 (as the
    integers the bf16 values hold)."""
    import numpy as np

    seed &= 0xFFFFFFFF
    raw, state = _lcg_stream(0x9E3779B9 ^ seed, 16 * 64)
    a32 = ((raw >> np.uint32(8)).astype(np.float32) / np.float32(16777216.0)) - np.float32(0.5)
    raw, _ = _lcg_stream(state, 64 * 16)
    b32 = ((raw >> np.uint32(8)).astype(np.float32) / np.float32(16777216.0)) - np.float32(0.5)
    raw, state = _lcg_stream(0x85EBCA6B ^ seed, 16 * 256)
    a8 = (raw >> np.uint32(24)).astype(np.uint8).view(np.int8).copy()
    raw, _ = _lcg_stream(state, 256 * 16)
    b8 = (raw >> np.uint32(24)).astype(np.uint8).view(np.int8).copy()
    a8[0], a8[1], b8[0], b8[16] = -128, 127, -128, 127

    def small(raw):
        mag = 1 + ((raw >> np.uint32(28)) & np.uint32(7)).astype(np.int32)
        return np.where((raw >> np.uint32(27)) & np.uint32(1), -mag, mag).astype(np.int32)

    raw, state = _lcg_stream(0xC2B2AE35 ^ seed, 32 * 64)
    a16 = small(raw)
    raw, _ = _lcg_stream(state, 64 * 32)
    b16 = small(raw)
    return {
        "f32": (a32.reshape(16, 64), b32.reshape(64, 16)),
        "i8": (a8.reshape(16, 256), b8.reshape(256, 16)),
        "bf16": (a16.reshape(32, 64), b16.reshape(64, 32)),
    }


def compute_expected_tiles(seed: int = 0) -> dict:
    """numpy mirror of the three expected tiles.  f32 is the k-ordered fmaf
    chain (``fmaf_chain``) — the CPU test compares this tile with the
    header's."""
    import numpy as np

    inputs = compute_inputs(seed)
    a32, b32 = inputs["f32"]
    acc, _ = fmaf_chain(a32, b32)
    a8, b8 = inputs["i8"]
    a16, b16 = inputs["bf16"]
    return {
        "f32": acc,
        "i8": a8.astype(np.int32) @ b8.astype(np.int32),
        "bf16": (a16 @ b16).astype(np.float32),
    }


def cu_key(xcc_id, hw_id):
    """(XCD, SE, SH, CU) of a record in one word (cro_cov_cu_key)."""
    return ((xcc_id & 0xF) << 16) | (hw_id & 0xFF00)


def decode_location(xcc_id, hw_id) -> dict:
    """numpy/int mirror of cro_cov_decode: HW_ID fields WAVE_ID 3:0,
    SIMD_ID 5:4, CU_ID 11:8, SH_ID 12, SE_ID 15:13; XCC_ID 3:0."""
    return {
        "xcd": xcc_id & 0xF,
        "se": (hw_id >> 13) & 0x7,
        "sh": (hw_id >> 12) & 0x1,
        "cu": (hw_id >> 8) & 0xF,
        "simd": (hw_id >> 4) & 0x3,
        "wave_slot": hw_id & 0xF,
    }


def decode_cu_key(key) -> dict:
    loc = decode_location(key >> 16, key & 0xFF00)
    return {k: loc[k] for k in ("xcd", "se", "sh", "cu")}


def aggregate_wave_records(records, tests):
    """numpy mirror of cro_wave_summarize (crocoverage.h) over a structured
    record array (or any mapping of equal-length uint32 arrays) of a stage
    whose fail-mask bits are ``tests``.  Returns what every stage's aggregate
    holds, with the per-test counts as ``bad_<test>``, and apart from it what
    only some hold: the OR of the fail masks and the keys of the CUs with a bad
    wave, in order of first appearance."""
    import numpy as np

    valid = np.asarray(records["valid"]) != 0
    xcc = np.asarray(records["xcc_id"])[valid].astype(np.int64)
    hw = np.asarray(records["hw_id"])[valid].astype(np.int64)
    mask = np.asarray(records["fail_mask"])[valid].astype(np.int64)
    keys = cu_key(xcc, hw)
    simd = (hw >> 4) & 0x3
    bad = mask != 0
    bad_keys = list(dict.fromkeys(keys[bad].tolist()))
    out = {"waves_run": int(valid.sum()), "waves_bad": int(bad.sum())}
    for bit, name in enumerate(tests):
        out[f"bad_{name}"] = int(((mask >> bit) & 1).sum())
    out.update({
        "first_bad_index": -1,
        "cus_seen": int(np.unique(keys).size),
        "xcds_seen": int(np.unique(xcc & 0xF).size),
        "simds_seen": int(np.unique(keys * 4 + simd).size),
        "cus_bad": len(bad_keys),
        "xcd": -1, "se": -1, "sh": -1, "cu": -1, "simd": -1,
        "first_fail_mask": 0, "n_bad": 0, "first_bad": 0xFFFFFFFF, "bits_bad": 0,
    })
    if bad.any():
        first = int(np.flatnonzero(valid)[np.flatnonzero(bad)[0]])
        loc = decode_location(int(records["xcc_id"][first]), int(records["hw_id"][first]))
        out.update({k: int(loc[k]) for k in ("xcd", "se", "sh", "cu", "simd")})
        out.update(
            first_bad_index=first,
            first_fail_mask=int(records["fail_mask"][first]),
            n_bad=int(records["n_bad"][first]),
            first_bad=int(records["first_bad"][first]),
            bits_bad=int(records["bits_bad"][first]),
        )
    return out, int(np.bitwise_or.reduce(mask)) if mask.size else 0, bad_keys


def aggregate_records(records) -> dict:
    """numpy mirror of cro_coverage_aggregate: aggregate_wave_records and the
    first eight bad CU keys."""
    out, _, bad_keys = aggregate_wave_records(records, ("f32", "i8", "bf16", "lds"))
    out.update(n_bad_cu_keys=min(len(bad_keys), 8), bad_cu_keys=bad_keys[:8])
    return out


def make_probe_fn(level: str = "quick", vram_bytes: int = 0, link_bytes: int = 0,
                  link_floor_gbps: float = 0.0, seed: int = 0, compute: bool = False,
                  compute_min_cu_fraction: float = 0.0, formats: bool = False,
                  formats_min_cu_fraction: float = 0.0, coherence: bool = False,
                  coherence_min_cu_fraction: float = 0.0, movement: bool = False,
                  movement_min_cu_fraction: float = 0.0, alu: bool = False,
                  alu_min_cu_fraction: float = 0.0):
    """AmdNodeOps probe hook for a probe level.

    ``quick`` is the rate/matrix-pipe gate.  ``deep`` runs it first and, only
    when it passed (a device that failed the quick gate is not stressed
    further), the data-integrity stage on the same ordinal; the result nests
    under ``"integrity"`` and ``ok`` is the AND of both.

    ``compute=True`` adds the compute-coverage stage to either level, between
    the two: quick, then compute, then (``deep``) integrity, stopping at the
    first stage that fails.  Its result nests under ``"compute"``; ``ok`` is
    the AND of the stages run and ``msg`` the failing stage's.

    ``formats=True`` adds the matrix-format stage (nodeops/formats.py) after
    the compute stage and before integrity, in the same way; its result nests
    under ``"formats"``.

    ``coherence=True`` adds the coherence stage (nodeops/coherence.py: the
    atomic units and cross-CU visibility) after the formats stage and before
    integrity, in the same way; its result nests under ``"coherence"``.

    ``movement=True`` adds the data-movement stage (nodeops/movement.py: the
    cross-lane, transposed-LDS-read and LDS-DMA paths) after the coherence
    stage and before integrity, in the same way; its result nests under
    ``"movement"``.

    ``alu=True`` adds the ALU stage (nodeops/alu.py: the vector and scalar
    ALUs and the transcendental consensus) after the movement stage and before
    integrity, in the same way; its result nests under ``"alu"``.  The order
    is quick, compute, formats, coherence, movement, alu, integrity.
    """
    if level not in PROBE_LEVELS:
        raise ValueError(f"unknown probe level {level!r} (expected one of {PROBE_LEVELS})")
    if (level == "quick" and not compute and not formats and not coherence and not movement
            and not alu):
        return probe_fn_for_nodeops

    def staged_probe(gpu) -> dict:
        dev = hip_device_for_bdf(gpu.pci_bdf)
        if dev is None:
            dev = 0
        result = run_probe(dev)
        if not result.get("ok"):
            return result
        if compute:
            stage = run_compute(dev, seed=seed, min_cu_fraction=compute_min_cu_fraction)
            result["compute"] = stage
            if not stage.get("ok"):
                result["ok"] = False
                result["msg"] = stage.get("msg", "compute probe failed")
                return result
        if formats:
            from .formats import run_formats

            stage = run_formats(dev, seed=seed, min_cu_fraction=formats_min_cu_fraction)
            result["formats"] = stage
            if not stage.get("ok"):
                result["ok"] = False
                result["msg"] = stage.get("msg", "formats probe failed")
                return result
        if coherence:
            from .coherence import run_coherence

            stage = run_coherence(dev, seed=seed, min_cu_fraction=coherence_min_cu_fraction)
            result["coherence"] = stage
            if not stage.get("ok"):
                result["ok"] = False
                result["msg"] = stage.get("msg", "coherence probe failed")
                return result
        if movement:
            from .movement import run_movement

            stage = run_movement(dev, seed=seed, min_cu_fraction=movement_min_cu_fraction)
            result["movement"] = stage
            if not stage.get("ok"):
                result["ok"] = False
                result["msg"] = stage.get("msg", "movement probe failed")
                return result
        if alu:
            from .alu import run_alu

            stage = run_alu(dev, seed=seed, min_cu_fraction=alu_min_cu_fraction)
            result["alu"] = stage
            if not stage.get("ok"):
                result["ok"] = False
                result["msg"] = stage.get("msg", "alu probe failed")
                return result
        if level == "deep":
            integrity = run_integrity(
                dev, vram_bytes=vram_bytes, link_bytes=link_bytes, seed=seed,
                link_floor_gbps=link_floor_gbps,
            )
            result["integrity"] = integrity
            if not integrity.get("ok"):
                result["ok"] = False
                result["msg"] = integrity.get("msg", "integrity probe failed")
        return result

    staged_probe.level = level
    staged_probe.compute = bool(compute)
    if formats:
        staged_probe.formats = True
    if coherence:
        staged_probe.coherence = True
    if movement:
        staged_probe.movement = True
    if alu:
        staged_probe.alu = True
    return staged_probe


def _compute_argv(compute, compute_min_cu_fraction) -> list:
    if not compute:
        return []
    argv = ["--compute"]
    if compute_min_cu_fraction:
        argv += ["--compute-min-cu-fraction", str(float(compute_min_cu_fraction))]
    return argv


def _formats_argv(formats, formats_min_cu_fraction) -> list:
    if not formats:
        return []
    argv = ["--formats"]
    if formats_min_cu_fraction:
        argv += ["--formats-min-cu-fraction", str(float(formats_min_cu_fraction))]
    return argv


def _coherence_argv(coherence, coherence_min_cu_fraction) -> list:
    if not coherence:
        return []
    argv = ["--coherence"]
    if coherence_min_cu_fraction:
        argv += ["--coherence-min-cu-fraction", str(float(coherence_min_cu_fraction))]
    return argv


def _movement_argv(movement, movement_min_cu_fraction) -> list:
    if not movement:
        return []
    argv = ["--movement"]
    if movement_min_cu_fraction:
        argv += ["--movement-min-cu-fraction", str(float(movement_min_cu_fraction))]
    return argv


def _alu_argv(alu, alu_min_cu_fraction) -> list:
    if not alu:
        return []
    argv = ["--alu"]
    if alu_min_cu_fraction:
        argv += ["--alu-min-cu-fraction", str(float(alu_min_cu_fraction))]
    return argv


def _deep_argv(level: str, vram_mib, link_mib, link_floor_gbps) -> list:
    if level == "quick":
        return []
    if level != "deep":
        raise ValueError(f"unknown probe level {level!r} (expected one of {PROBE_LEVELS})")
    argv = ["--deep"]
    if vram_mib:
        argv += ["--vram-mib", str(int(vram_mib))]
    if link_mib:
        argv += ["--link-mib", str(int(link_mib))]
    if link_floor_gbps:
        argv += ["--link-floor-gbps", str(float(link_floor_gbps))]
    return argv


def probe_via_exec(execer, node: str, gpu, argv_prefix=None, level: str = "quick",
                   vram_mib=None, link_mib=None, link_floor_gbps=0, compute: bool = False,
                   compute_min_cu_fraction=0, formats: bool = False,
                   formats_min_cu_fraction=0, coherence: bool = False,
                   coherence_min_cu_fraction=0, movement: bool = False,
                   movement_min_cu_fraction=0, alu: bool = False,
                   alu_min_cu_fraction=0) -> dict:
    """Health probe through the node agent (``croagent probe --bdf``) — the
    cluster shape where controllers run off-node and reach hardware only
    through the NodeExec seam.  Returns the same dict shape as run_probe
    (at level ``deep``: as make_probe_fn("deep"), via ``croagent probe
    --deep`` and the size options given; with ``compute``: as
    make_probe_fn(..., compute=True), via ``--compute``; with ``formats``:
    via ``--formats``; with ``coherence``: via ``--coherence``; with
    ``movement``: via ``--movement``; with ``alu``: via ``--alu``).

    ``argv_prefix`` wraps the command for the container-driver arm (e.g.
    ``["chroot", "/run/amdgpu-driver"]`` so the probe runs against the
    driver container's ROCm userspace — the nvidia-smi-through-chroot
    analog, gpus.go:566-749).
    """
    import json as _json

    argv = list(argv_prefix or []) + ["croagent", "probe", "--bdf", gpu.pci_bdf]
    argv += _deep_argv(level, vram_mib, link_mib, link_floor_gbps)
    argv += _compute_argv(compute, compute_min_cu_fraction)
    argv += _formats_argv(formats, formats_min_cu_fraction)
    argv += _coherence_argv(coherence, coherence_min_cu_fraction)
    argv += _movement_argv(movement, movement_min_cu_fraction)
    argv += _alu_argv(alu, alu_min_cu_fraction)
    rc, out, err = execer.run(node, argv, timeout=300)
    if rc != 0 and not out.strip():
        return {"ok": False, "rc": rc, "msg": err.strip() or "croagent probe failed"}
    try:
        return _json.loads(out)
    except ValueError:
        return {"ok": False, "rc": rc, "msg": f"unparseable probe output: {out[:200]}"}


def make_exec_probe_fn(execer, node: str, argv_prefix_fn=None, level: str = "quick",
                       vram_mib=None, link_mib=None, link_floor_gbps=0, compute: bool = False,
                       compute_min_cu_fraction=0, formats: bool = False,
                       formats_min_cu_fraction=0, coherence: bool = False,
                       coherence_min_cu_fraction=0, movement: bool = False,
                       movement_min_cu_fraction=0, alu: bool = False,
                       alu_min_cu_fraction=0):
    """AmdNodeOps probe hook bound to a NodeExec (local or remote agent).

    ``argv_prefix_fn()`` is resolved per probe so a driver-mode change
    (DeviceConfig applied mid-flight) switches the chroot arm without a
    rebuild — pass ``lambda: ops.probe_argv_prefix(node)``.
    """
    _deep_argv(level, vram_mib, link_mib, link_floor_gbps)  # reject a bad level now

    # a stage that is off passes no keyword of its own
    stages = {}
    if formats:
        stages.update(formats=True, formats_min_cu_fraction=formats_min_cu_fraction)
    if coherence:
        stages.update(coherence=True, coherence_min_cu_fraction=coherence_min_cu_fraction)
    if movement:
        stages.update(movement=True, movement_min_cu_fraction=movement_min_cu_fraction)
    if alu:
        stages.update(alu=True, alu_min_cu_fraction=alu_min_cu_fraction)

    def probe(gpu):
        prefix = argv_prefix_fn() if argv_prefix_fn else None
        return probe_via_exec(
            execer, node, gpu, argv_prefix=prefix, level=level, vram_mib=vram_mib,
            link_mib=link_mib, link_floor_gbps=link_floor_gbps, compute=compute,
            compute_min_cu_fraction=compute_min_cu_fraction, **stages,
        )

    return probe
