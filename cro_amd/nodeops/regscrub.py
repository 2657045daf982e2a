"""ctypes wrapper for the register scrub stage (cro_amd/hip/regscrub.hip →
libcroregscrub.so): clear and verify the vector register file of every SIMD
of every CU before a GPU is drained.

Fails LOUDLY on a GPU node without the compiled library, as the VRAM and LDS
scrubs' wrappers do: a site that asked for the register scrub must never
detach without it and not hear of it.  What the stage covers (VGPRs from
``first_vgpr`` up and all AGPRs, censused and verified; the VGPRs below
overwritten only) and what it does not (SGPRs, trap-handler and hardware
state registers) is in cro_amd/hip/croregscrub.h.
"""

from __future__ import annotations

import ctypes
import os
from typing import Optional

from .probe import _gpu_present, _result_dict

_LIB_PATH = os.path.join(os.path.dirname(__file__), "..", "hip", "libcroregscrub.so")

FIRST_VGPR = 16  # the first covered VGPR
REGS_PER_LANE = (256 - FIRST_VGPR) + 256  # covered: VGPRs first, then AGPRs
WAVE_WORDS = REGS_PER_LANE * 64
WAVES = 4  # per workgroup, one per SIMD
NO_WORD = (1 << 32) - 1  # first_dirty_word / first_bad_word when there is none


class CroRegScrubOpts(ctypes.Structure):
    """Mirror of ``struct CroRegScrubOpts`` (cro_amd/hip/croregscrub.h)."""

    _fields_ = [
        ("grid", ctypes.c_int),
        ("max_rounds", ctypes.c_int),
        ("skip_recheck", ctypes.c_int),
        ("fill_word", ctypes.c_uint),
        ("selftest_mode", ctypes.c_int),
        ("selftest_pattern", ctypes.c_uint),
        ("selftest_wave", ctypes.c_int),
        ("selftest_word", ctypes.c_uint),
        ("selftest_bit", ctypes.c_int),
        ("reserved", ctypes.c_int),
        ("min_simd_fraction", ctypes.c_double),
    ]


class CroRegScrubResult(ctypes.Structure):
    """Mirror of ``struct CroRegScrubResult`` (cro_amd/hip/croregscrub.h)."""

    _fields_ = [
        ("ok", ctypes.c_int),
        ("rc", ctypes.c_int),
        ("simds_expected", ctypes.c_int),
        ("simds_seen", ctypes.c_int),
        ("cus_seen", ctypes.c_int),
        ("xcds_seen", ctypes.c_int),
        ("rounds", ctypes.c_int),
        ("grid", ctypes.c_int),
        ("first_vgpr", ctypes.c_int),
        ("regs_per_lane", ctypes.c_int),
        ("waves", ctypes.c_ulonglong),
        ("bytes_scrubbed", ctypes.c_ulonglong),
        ("dirty_words_before", ctypes.c_ulonglong),
        ("dirty_waves", ctypes.c_ulonglong),
        ("n_bad", ctypes.c_ulonglong),
        ("recheck_dirty_words", ctypes.c_ulonglong),
        ("first_dirty_word", ctypes.c_uint),
        ("first_bad_word", ctypes.c_uint),
        ("bits_bad", ctypes.c_uint),
        ("bad_waves", ctypes.c_int),
        ("xcd", ctypes.c_int),
        ("se", ctypes.c_int),
        ("sh", ctypes.c_int),
        ("cu", ctypes.c_int),
        ("simd", ctypes.c_int),
        ("wave", ctypes.c_int),
        ("gpu_ms", ctypes.c_double),
        ("t_total_ms", ctypes.c_double),
        ("msg", ctypes.c_char * 256),
    ]


class CroRegScrubRecord(ctypes.Structure):
    """Mirror of ``struct CroRegScrubRecord``: one per wave and dispatch."""

    _fields_ = [(name, ctypes.c_uint32) for name in (
        "xcc_id", "hw_id", "dirty_lanes", "first_dirty", "n_bad", "first_bad", "bits_bad",
        "valid")]


_lib = None


def load_reg_scrub_library(required: Optional[bool] = None) -> Optional[ctypes.CDLL]:
    """Load libcroregscrub.so.  required=None → required iff a GPU is present."""
    global _lib
    if _lib is not None:
        return _lib
    if required is None:
        required = _gpu_present()
    path = os.path.abspath(_LIB_PATH)
    if not os.path.exists(path):
        if required:
            raise RuntimeError(
                f"libcroregscrub.so missing at {path} on a GPU node — build it with "
                "`python -m cro_amd.hip.build` (hipcc --offload-arch=gfx950)"
            )
        return None
    lib = ctypes.CDLL(path)
    lib.cro_reg_scrub_run.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroRegScrubOpts), ctypes.POINTER(CroRegScrubResult),
    ]
    lib.cro_reg_scrub_run.restype = ctypes.c_int
    lib.cro_reg_scrub_run_records.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroRegScrubOpts), ctypes.POINTER(CroRegScrubResult),
        ctypes.POINTER(CroRegScrubRecord), ctypes.c_int,
    ]
    lib.cro_reg_scrub_run_records.restype = ctypes.c_int
    _lib = lib
    return lib


def _reg_scrub_opts(grid=0, max_rounds=0, skip_recheck=0, fill_word=0, min_simd_fraction=0.0,
                    selftest_mode=0, selftest_pattern=0, selftest_wave=0, selftest_word=0,
                    selftest_bit=0) -> CroRegScrubOpts:
    return CroRegScrubOpts(
        grid=int(grid), max_rounds=int(max_rounds), skip_recheck=int(skip_recheck),
        fill_word=int(fill_word) & 0xFFFFFFFF, selftest_mode=int(selftest_mode),
        selftest_pattern=int(selftest_pattern) & 0xFFFFFFFF, selftest_wave=int(selftest_wave),
        selftest_word=int(selftest_word) & 0xFFFFFFFF, selftest_bit=int(selftest_bit),
        min_simd_fraction=float(min_simd_fraction),
    )


def run_reg_scrub(device: int = 0, **opts) -> dict:
    """Place one wave on every SIMD of ``device``; each counts the words of its
    vector register file that differ from ``fill_word``, fills them and reads
    them back, and a further dispatch counts once more
    (``recheck_dirty_words``).  Options as ``struct CroRegScrubOpts``; zero
    takes the library default.  Residue always fails (rc -44); the SIMDs
    reached are reported as ``simds_seen`` of ``simds_expected`` and gate only
    when ``min_simd_fraction`` > 0 (rc -45).  The ``selftest_*`` options are
    for tests."""
    lib = load_reg_scrub_library(required=True)
    c_opts = _reg_scrub_opts(**opts)
    res = CroRegScrubResult()
    rc = lib.cro_reg_scrub_run(device, ctypes.byref(c_opts), ctypes.byref(res))
    return _result_dict(res, rc)


def run_reg_scrub_records(device: int = 0, max_records: int = 8192, **opts):
    """run_reg_scrub, and the rounds' per-wave records as a list of dicts in
    dispatch order, four per workgroup (at most ``max_records``).  For tests."""
    lib = load_reg_scrub_library(required=True)
    c_opts = _reg_scrub_opts(**opts)
    res = CroRegScrubResult()
    records = (CroRegScrubRecord * max_records)()
    rc = lib.cro_reg_scrub_run_records(device, ctypes.byref(c_opts), ctypes.byref(res), records,
                                       max_records)
    n = min(int(res.waves), max_records)
    names = [name for name, _ in CroRegScrubRecord._fields_]
    return _result_dict(res, rc), [{k: getattr(r, k) for k in names} for r in records[:n]]
