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


class CroIntegrityOpts(ctypes.Structure):
    """Mirror of ``struct CroIntegrityOpts`` (cro_amd/hip/croprobe.h)."""

    _fields_ = [
        ("vram_bytes", ctypes.c_longlong),
        ("link_bytes", ctypes.c_longlong),
        ("chunk_bytes", ctypes.c_longlong),
        ("seed", ctypes.c_uint),
        ("reserved", ctypes.c_int),
        ("link_floor_gbps", ctypes.c_double),
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
        ctypes.c_ulonglong, ctypes.c_ulonglong, u32p,
    ]
    lib.cro_probe_pattern_fill.restype = ctypes.c_int
    lib.cro_probe_pattern_verify.argtypes = [
        ctypes.c_int, ctypes.c_uint, ctypes.c_int,
        ctypes.c_ulonglong, ctypes.c_ulonglong, u32p, u64p, u64p, u32p,
    ]
    lib.cro_probe_pattern_verify.restype = ctypes.c_int
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


def run_probe(device: int = 0) -> dict:
    lib = load_library(required=True)
    res = CroProbeResult()
    rc = lib.cro_probe_run(device, ctypes.byref(res))
    return {
        "ok": bool(res.ok) and rc == 0,
        "rc": rc,
        "mfma_f32_exact": bool(res.mfma_f32_exact),
        "hbm_gbps": res.hbm_gbps,
        "bf16_tflops": res.bf16_tflops,
        "vram_total": res.vram_total,
        "vram_free": res.vram_free,
        "t_setup_ms": res.t_setup_ms,
        "t_mfma_ms": res.t_mfma_ms,
        "t_bw_ms": res.t_bw_ms,
        "t_bf16_ms": res.t_bf16_ms,
        "gcn_arch": res.gcn_arch.decode(errors="replace"),
        "msg": res.msg.decode(errors="replace"),
    }


def probe_fn_for_nodeops(gpu) -> dict:
    """AmdNodeOps probe hook: GPUDevice → probe result on the right ordinal."""
    dev = hip_device_for_bdf(gpu.pci_bdf)
    if dev is None:
        dev = 0
    return run_probe(dev)


def run_integrity(
    device: int = 0,
    vram_bytes: int = 0,
    link_bytes: int = 0,
    seed: int = 0,
    link_floor_gbps: float = 0.0,
    chunk_bytes: int = 0,
) -> dict:
    """Deep probe: verify the content of ``vram_bytes`` of VRAM and of
    ``link_bytes`` moved across the host link in both directions, by copy
    engine and by shader (cro_amd/hip/integrity.hip).  Zero sizes take the
    library defaults.  Gates on data only, unless ``link_floor_gbps`` > 0."""
    lib = load_library(required=True)
    opts = CroIntegrityOpts(
        vram_bytes=int(vram_bytes),
        link_bytes=int(link_bytes),
        chunk_bytes=int(chunk_bytes),
        seed=int(seed) & 0xFFFFFFFF,
        link_floor_gbps=float(link_floor_gbps),
    )
    res = CroIntegrityResult()
    rc = lib.cro_probe_integrity(device, ctypes.byref(opts), ctypes.byref(res))
    out = {"ok": bool(res.ok) and rc == 0, "rc": rc}
    for name, _ in CroIntegrityResult._fields_[2:]:
        value = getattr(res, name)
        out[name] = value.decode(errors="replace") if isinstance(value, bytes) else value
    return out


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
    """Run the fill kernel on ``n_words`` of VRAM and return them (uint32)."""
    import numpy as np

    lib = load_library(required=True)
    out = np.zeros(n_words, dtype=np.uint32)
    rc = lib.cro_probe_pattern_fill(
        device, seed & 0xFFFFFFFF, 1 if invert else 0, base_word, n_words,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)),
    )
    if rc != 0:
        raise RuntimeError(f"cro_probe_pattern_fill failed: rc={rc}")
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


def make_probe_fn(level: str = "quick", vram_bytes: int = 0, link_bytes: int = 0,
                  link_floor_gbps: float = 0.0, seed: int = 0):
    """AmdNodeOps probe hook for a probe level.

    ``quick`` is the rate/matrix-pipe gate.  ``deep`` runs it first and, only
    when it passed (a device that failed the quick gate is not stressed
    further), the data-integrity stage on the same ordinal; the result nests
    under ``"integrity"`` and ``ok`` is the AND of both.
    """
    if level == "quick":
        return probe_fn_for_nodeops
    if level != "deep":
        raise ValueError(f"unknown probe level {level!r} (expected one of {PROBE_LEVELS})")

    def deep_probe(gpu) -> dict:
        dev = hip_device_for_bdf(gpu.pci_bdf)
        if dev is None:
            dev = 0
        result = run_probe(dev)
        if not result.get("ok"):
            return result
        integrity = run_integrity(
            dev, vram_bytes=vram_bytes, link_bytes=link_bytes, seed=seed,
            link_floor_gbps=link_floor_gbps,
        )
        result["integrity"] = integrity
        if not integrity.get("ok"):
            result["ok"] = False
            result["msg"] = integrity.get("msg", "integrity probe failed")
        return result

    deep_probe.level = "deep"
    return deep_probe


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
                   vram_mib=None, link_mib=None, link_floor_gbps=0) -> dict:
    """Health probe through the node agent (``croagent probe --bdf``) — the
    cluster shape where controllers run off-node and reach hardware only
    through the NodeExec seam.  Returns the same dict shape as run_probe
    (at level ``deep``: as make_probe_fn("deep"), via ``croagent probe
    --deep`` and the size options given).

    ``argv_prefix`` wraps the command for the container-driver arm (e.g.
    ``["chroot", "/run/amdgpu-driver"]`` so the probe runs against the
    driver container's ROCm userspace — the nvidia-smi-through-chroot
    analog, gpus.go:566-749).
    """
    import json as _json

    argv = list(argv_prefix or []) + ["croagent", "probe", "--bdf", gpu.pci_bdf]
    argv += _deep_argv(level, vram_mib, link_mib, link_floor_gbps)
    rc, out, err = execer.run(node, argv, timeout=300)
    if rc != 0 and not out.strip():
        return {"ok": False, "rc": rc, "msg": err.strip() or "croagent probe failed"}
    try:
        return _json.loads(out)
    except ValueError:
        return {"ok": False, "rc": rc, "msg": f"unparseable probe output: {out[:200]}"}


def make_exec_probe_fn(execer, node: str, argv_prefix_fn=None, level: str = "quick",
                       vram_mib=None, link_mib=None, link_floor_gbps=0):
    """AmdNodeOps probe hook bound to a NodeExec (local or remote agent).

    ``argv_prefix_fn()`` is resolved per probe so a driver-mode change
    (DeviceConfig applied mid-flight) switches the chroot arm without a
    rebuild — pass ``lambda: ops.probe_argv_prefix(node)``.
    """
    _deep_argv(level, vram_mib, link_mib, link_floor_gbps)  # reject a bad level now

    def probe(gpu):
        prefix = argv_prefix_fn() if argv_prefix_fn else None
        return probe_via_exec(
            execer, node, gpu, argv_prefix=prefix, level=level, vram_mib=vram_mib,
            link_mib=link_mib, link_floor_gbps=link_floor_gbps,
        )

    return probe
