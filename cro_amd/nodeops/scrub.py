"""ctypes wrapper for the scrub-on-detach stage (cro_amd/hip/scrub.hip →
libcroscrub.so): overwrite and verify a GPU's VRAM before it is drained.

Fails LOUDLY on a GPU node without the compiled library, as the probe
wrapper does: a site that asked for a scrub must never detach unscrubbed
without hearing of it.  What the scrub covers and what it does not is in
cro_amd/hip/croscrub.h.
"""

from __future__ import annotations

import ctypes
import os
from typing import Optional

from .probe import _gpu_present, _result_dict, hip_device_for_bdf

_LIB_PATH = os.path.join(os.path.dirname(__file__), "..", "hip", "libcroscrub.so")


class CroScrubOpts(ctypes.Structure):
    """Mirror of ``struct CroScrubOpts`` (cro_amd/hip/croscrub.h)."""

    _fields_ = [
        ("max_bytes", ctypes.c_longlong),
        ("chunk_bytes", ctypes.c_longlong),
        ("reserve_bytes", ctypes.c_longlong),
        ("fill_word", ctypes.c_uint),
        ("selftest_mode", ctypes.c_int),
        ("min_fraction", ctypes.c_double),
        ("selftest_bit", ctypes.c_int),
        ("selftest_refuse_at", ctypes.c_int),
        ("selftest_word", ctypes.c_ulonglong),
    ]


class CroScrubResult(ctypes.Structure):
    """Mirror of ``struct CroScrubResult`` (cro_amd/hip/croscrub.h)."""

    _fields_ = [
        ("ok", ctypes.c_int),
        ("rc", ctypes.c_int),
        ("vram_total", ctypes.c_longlong),
        ("vram_free_before", ctypes.c_longlong),
        ("bytes_target", ctypes.c_longlong),
        ("bytes_scrubbed", ctypes.c_longlong),
        ("bytes_verified", ctypes.c_longlong),
        ("chunks", ctypes.c_int),
        ("alloc_refusals", ctypes.c_int),
        ("dirty_words_before", ctypes.c_ulonglong),
        ("n_bad", ctypes.c_ulonglong),
        ("first_bad_byte", ctypes.c_ulonglong),
        ("bits_bad", ctypes.c_uint),
        ("first_bad_got", ctypes.c_uint),
        ("fraction", ctypes.c_double),
        ("fill_gbps", ctypes.c_double),
        ("verify_gbps", ctypes.c_double),
        ("census_gbps", ctypes.c_double),
        ("t_alloc_ms", ctypes.c_double),
        ("t_total_ms", ctypes.c_double),
        ("msg", ctypes.c_char * 256),
    ]


NO_BAD_WORD = (1 << 64) - 1  # first_bad / first_bad_byte when nothing is bad

_lib = None


def load_scrub_library(required: Optional[bool] = None) -> Optional[ctypes.CDLL]:
    """Load libcroscrub.so.  required=None → required iff a GPU is present."""
    global _lib
    if _lib is not None:
        return _lib
    if required is None:
        required = _gpu_present()
    path = os.path.abspath(_LIB_PATH)
    if not os.path.exists(path):
        if required:
            raise RuntimeError(
                f"libcroscrub.so missing at {path} on a GPU node — build it with "
                "`python -m cro_amd.hip.build` (hipcc --offload-arch=gfx950)"
            )
        return None
    lib = ctypes.CDLL(path)
    lib.cro_scrub_run.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroScrubOpts), ctypes.POINTER(CroScrubResult),
    ]
    lib.cro_scrub_run.restype = ctypes.c_int
    u32p = ctypes.POINTER(ctypes.c_uint)
    u64p = ctypes.POINTER(ctypes.c_ulonglong)
    lib.cro_scrub_fill.argtypes = [
        ctypes.c_int, ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_int, u32p,
        ctypes.POINTER(ctypes.c_int),
    ]
    lib.cro_scrub_fill.restype = ctypes.c_int
    lib.cro_scrub_verify.argtypes = [
        ctypes.c_int, u32p, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_uint,
        ctypes.c_int, u64p, u64p, u32p,
    ]
    lib.cro_scrub_verify.restype = ctypes.c_int
    lib.cro_scrub_grid_pass_words.argtypes = []
    lib.cro_scrub_grid_pass_words.restype = ctypes.c_ulonglong
    _lib = lib
    return lib


def _scrub_opts(max_bytes=0, chunk_bytes=0, reserve_bytes=0, fill_word=0, min_fraction=0.0,
                selftest_mode=0, selftest_word=0, selftest_bit=0,
                selftest_refuse_at=0) -> CroScrubOpts:
    return CroScrubOpts(
        max_bytes=int(max_bytes), chunk_bytes=int(chunk_bytes),
        reserve_bytes=int(reserve_bytes), fill_word=int(fill_word) & 0xFFFFFFFF,
        min_fraction=float(min_fraction), selftest_mode=int(selftest_mode),
        selftest_bit=int(selftest_bit), selftest_refuse_at=int(selftest_refuse_at),
        selftest_word=int(selftest_word),
    )


def run_scrub(device: int = 0, **opts) -> dict:
    """Take all the VRAM of ``device`` the driver hands over (at most
    ``max_bytes`` when given, leaving ``reserve_bytes`` free), count the words
    in it that differ from ``fill_word``, fill it and read every word back.
    Options as ``struct CroScrubOpts``; zero takes the library default.
    Residue after the fill always fails (rc -40); the covered share of VRAM is
    reported as ``fraction`` and gates only when ``min_fraction`` > 0 (rc -41).
    The ``selftest_*`` options are for tests."""
    lib = load_scrub_library(required=True)
    c_opts = _scrub_opts(**opts)
    res = CroScrubResult()
    rc = lib.cro_scrub_run(device, ctypes.byref(c_opts), ctypes.byref(res))
    return _result_dict(res, rc)


# -- raw kernel entries and their reference, for tests ----------------------------


def grid_pass_words() -> int:
    """Words one pass of the production grid covers."""
    return int(load_scrub_library(required=True).cro_scrub_grid_pass_words())


def scrub_fill(device: int, n_words: int, fill_word: int, grid_blocks: int = 0):
    """Run the fill kernel on ``n_words`` of VRAM and return them (uint32).
    Raises when the kernel wrote anything outside them (the slack of the last
    vector and a guard band on either side are preset and read back)."""
    import numpy as np

    lib = load_scrub_library(required=True)
    out = np.zeros(n_words, dtype=np.uint32)
    guard_ok = ctypes.c_int(0)
    rc = lib.cro_scrub_fill(
        device, n_words, fill_word & 0xFFFFFFFF, int(grid_blocks),
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), ctypes.byref(guard_ok),
    )
    if rc != 0:
        raise RuntimeError(f"cro_scrub_fill failed: rc={rc}")
    if not guard_ok.value:
        raise RuntimeError(f"cro_scrub_fill wrote outside its {n_words} words")
    return out


def scrub_verify(device: int, words, fill_word: int, base_word: int = 0,
                 grid_blocks: int = 0) -> dict:
    """Upload ``words`` (uint32 array) and run the verify kernel on them."""
    import numpy as np

    lib = load_scrub_library(required=True)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    n_bad = ctypes.c_ulonglong()
    first_bad = ctypes.c_ulonglong()
    bits_bad = ctypes.c_uint()
    rc = lib.cro_scrub_verify(
        device, words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), words.size, base_word,
        fill_word & 0xFFFFFFFF, int(grid_blocks),
        ctypes.byref(n_bad), ctypes.byref(first_bad), ctypes.byref(bits_bad),
    )
    if rc != 0:
        raise RuntimeError(f"cro_scrub_verify failed: rc={rc}")
    return {"n_bad": n_bad.value, "first_bad": first_bad.value, "bits_bad": bits_bad.value}


def scrub_report(words, fill_word: int, base_word: int = 0) -> dict:
    """numpy reference of the verify kernel's report over ``words``."""
    import numpy as np

    diff = np.ascontiguousarray(words, dtype=np.uint32) ^ np.uint32(fill_word & 0xFFFFFFFF)
    bad = np.flatnonzero(diff)
    return {
        "n_bad": int(bad.size),
        "first_bad": base_word + int(bad[0]) if bad.size else NO_BAD_WORD,
        "bits_bad": int(np.bitwise_or.reduce(diff)) if diff.size else 0,
    }


# -- node-ops hooks ---------------------------------------------------------------


def merge_lds_result(vram: dict, lds: dict) -> dict:
    """The VRAM scrub's result with the LDS scrub's nested under ``"lds"``:
    ``ok`` only if both passed; ``rc`` and ``msg`` are the VRAM scrub's when
    that failed, else the LDS scrub's."""
    out = dict(vram)
    out["lds"] = lds
    out["ok"] = bool(vram.get("ok")) and bool(lds.get("ok"))
    if vram.get("ok"):
        out["rc"] = lds.get("rc")
        out["msg"] = lds.get("msg", "")
    return out


def merge_regs_result(merged: dict, regs: dict) -> dict:
    """``merged`` (the VRAM scrub's result, the LDS scrub's already merged in
    when that ran) with the register scrub's nested under ``"regs"``, after
    ``"lds"``: ``ok`` only if every stage passed; ``rc`` and ``msg`` stay those
    of the first stage that failed, else become the register scrub's."""
    out = dict(merged)
    out["regs"] = regs
    out["ok"] = bool(merged.get("ok")) and bool(regs.get("ok"))
    if merged.get("ok"):
        out["rc"] = regs.get("rc")
        out["msg"] = regs.get("msg", "")
    return out


def make_scrub_fn(max_bytes: int = 0, reserve_bytes: int = 0, min_fraction: float = 0.0,
                  lds: bool = False, lds_min_cu_fraction: float = 0.0, regs: bool = False,
                  regs_min_simd_fraction: float = 0.0):
    """AmdNodeOps scrub hook: GPUDevice → scrub result on the right ordinal.
    ``lds``: the LDS scrub (nodeops/ldsscrub.py) runs after the VRAM scrub and
    its result is merged in (merge_lds_result).  ``regs``: the register scrub
    (nodeops/regscrub.py) runs after those and is merged in last
    (merge_regs_result)."""

    def scrub(gpu) -> dict:
        dev = hip_device_for_bdf(gpu.pci_bdf)
        if dev is None:
            dev = 0
        result = run_scrub(dev, max_bytes=max_bytes, reserve_bytes=reserve_bytes,
                           min_fraction=min_fraction)
        if lds:
            from . import ldsscrub

            result = merge_lds_result(
                result, ldsscrub.run_lds_scrub(dev, min_cu_fraction=lds_min_cu_fraction))
        if regs:
            from . import regscrub

            result = merge_regs_result(
                result, regscrub.run_reg_scrub(dev, min_simd_fraction=regs_min_simd_fraction))
        return result

    return scrub


def scrub_via_exec(execer, node: str, gpu, argv_prefix=None, max_mib=None, reserve_mib=None,
                   min_fraction=0, lds=False, lds_min_cu_fraction=0.0, regs=False,
                   regs_min_simd_fraction=0.0) -> dict:
    """Scrub through the node agent (``croagent scrub --bdf``), for
    controllers that run off-node.  Returns the same dict shape as run_scrub
    (with ``lds`` and ``regs``: as make_scrub_fn's, merged by the agent);
    ``argv_prefix`` as in probe.probe_via_exec."""
    import json as _json

    argv = list(argv_prefix or []) + ["croagent", "scrub", "--bdf", gpu.pci_bdf]
    if max_mib:
        argv += ["--max-mib", str(int(max_mib))]
    if reserve_mib:
        argv += ["--reserve-mib", str(int(reserve_mib))]
    if min_fraction:
        argv += ["--min-fraction", str(float(min_fraction))]
    if lds:
        argv += ["--lds"]
        if lds_min_cu_fraction:
            argv += ["--lds-min-cu-fraction", str(float(lds_min_cu_fraction))]
    if regs:
        argv += ["--regs"]
        if regs_min_simd_fraction:
            argv += ["--regs-min-simd-fraction", str(float(regs_min_simd_fraction))]
    rc, out, err = execer.run(node, argv, timeout=300)
    if not out.strip():
        return {"ok": False, "rc": rc, "msg": err.strip() or "croagent scrub failed"}
    try:
        result = _json.loads(out)
    except ValueError:
        return {"ok": False, "rc": rc, "msg": f"unparseable scrub output: {out[:200]}"}
    if not isinstance(result, dict):
        return {"ok": False, "rc": rc, "msg": f"unparseable scrub output: {out[:200]}"}
    return result


def make_exec_scrub_fn(execer, node: str, argv_prefix_fn=None, max_mib=None, reserve_mib=None,
                       min_fraction=0, lds=False, lds_min_cu_fraction=0.0, regs=False,
                       regs_min_simd_fraction=0.0):
    """AmdNodeOps scrub hook bound to a NodeExec (local or remote agent);
    ``argv_prefix_fn`` as in probe.make_exec_probe_fn."""

    def scrub(gpu):
        prefix = argv_prefix_fn() if argv_prefix_fn else None
        # a stage that is off passes no keyword of its own: the call is then
        # exactly what it was before the stage existed
        stages = {}
        if lds:
            stages.update(lds=True, lds_min_cu_fraction=lds_min_cu_fraction)
        if regs:
            stages.update(regs=True, regs_min_simd_fraction=regs_min_simd_fraction)
        return scrub_via_exec(execer, node, gpu, argv_prefix=prefix, max_mib=max_mib,
                              reserve_mib=reserve_mib, min_fraction=min_fraction, **stages)

    return scrub
