"""ctypes wrapper for the LDS scrub stage (cro_amd/hip/ldsscrub.hip →
libcroldsscrub.so): clear and verify every CU's LDS before a GPU is drained.

Fails LOUDLY on a GPU node without the compiled library, as the VRAM scrub's
wrapper does: a site that asked for the LDS scrub must never detach without
it and not hear of it.  What the stage covers and what it does not (registers:
the vector registers are nodeops/regscrub.py's stage) is in
cro_amd/hip/croldsscrub.h.
"""

from __future__ import annotations

import ctypes
import os
from typing import Optional

from .probe import _gpu_present, _result_dict

_LIB_PATH = os.path.join(os.path.dirname(__file__), "..", "hip", "libcroldsscrub.so")

LDS_BYTES = 163840  # one CU's whole LDS
GUARD_WORD = 0xA5A5A5A5  # self-test: preset of the words that are not marched
NO_WORD = (1 << 32) - 1  # first_dirty_word / first_bad_word when there is none


class CroLdsScrubOpts(ctypes.Structure):
    """Mirror of ``struct CroLdsScrubOpts`` (cro_amd/hip/croldsscrub.h)."""

    _fields_ = [
        ("lds_bytes", ctypes.c_int),
        ("grid", ctypes.c_int),
        ("max_rounds", ctypes.c_int),
        ("skip_recheck", ctypes.c_int),
        ("fill_word", ctypes.c_uint),
        ("selftest_mode", ctypes.c_int),
        ("selftest_pattern", ctypes.c_uint),
        ("selftest_word", ctypes.c_uint),
        ("selftest_bit", ctypes.c_int),
        ("reserved", ctypes.c_int),
        ("min_cu_fraction", ctypes.c_double),
    ]


class CroLdsScrubResult(ctypes.Structure):
    """Mirror of ``struct CroLdsScrubResult`` (cro_amd/hip/croldsscrub.h)."""

    _fields_ = [
        ("ok", ctypes.c_int),
        ("rc", ctypes.c_int),
        ("cus_expected", ctypes.c_int),
        ("cus_seen", ctypes.c_int),
        ("xcds_seen", ctypes.c_int),
        ("rounds", ctypes.c_int),
        ("lds_bytes", ctypes.c_int),
        ("grid", ctypes.c_int),
        ("workgroups", ctypes.c_ulonglong),
        ("bytes_scrubbed", ctypes.c_ulonglong),
        ("dirty_words_before", ctypes.c_ulonglong),
        ("dirty_workgroups", ctypes.c_ulonglong),
        ("n_bad", ctypes.c_ulonglong),
        ("guard_bad", ctypes.c_ulonglong),
        ("recheck_dirty_words", ctypes.c_ulonglong),
        ("first_dirty_word", ctypes.c_uint),
        ("first_bad_word", ctypes.c_uint),
        ("bits_bad", ctypes.c_uint),
        ("bad_workgroups", ctypes.c_int),
        ("xcd", ctypes.c_int),
        ("se", ctypes.c_int),
        ("sh", ctypes.c_int),
        ("cu", ctypes.c_int),
        ("gpu_ms", ctypes.c_double),
        ("t_total_ms", ctypes.c_double),
        ("msg", ctypes.c_char * 256),
    ]


class CroLdsScrubRecord(ctypes.Structure):
    """Mirror of ``struct CroLdsScrubRecord``: one per workgroup and dispatch."""

    _fields_ = [(name, ctypes.c_uint32) for name in (
        "xcc_id", "hw_id", "dirty_words", "first_dirty", "n_bad", "first_bad", "bits_bad",
        "guard_bad", "valid", "reserved")]


_lib = None


def load_lds_scrub_library(required: Optional[bool] = None) -> Optional[ctypes.CDLL]:
    """Load libcroldsscrub.so.  required=None → required iff a GPU is present."""
    global _lib
    if _lib is not None:
        return _lib
    if required is None:
        required = _gpu_present()
    path = os.path.abspath(_LIB_PATH)
    if not os.path.exists(path):
        if required:
            raise RuntimeError(
                f"libcroldsscrub.so missing at {path} on a GPU node — build it with "
                "`python -m cro_amd.hip.build` (hipcc --offload-arch=gfx950)"
            )
        return None
    lib = ctypes.CDLL(path)
    lib.cro_lds_scrub_run.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroLdsScrubOpts), ctypes.POINTER(CroLdsScrubResult),
    ]
    lib.cro_lds_scrub_run.restype = ctypes.c_int
    lib.cro_lds_scrub_run_records.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroLdsScrubOpts), ctypes.POINTER(CroLdsScrubResult),
        ctypes.POINTER(CroLdsScrubRecord), ctypes.c_int,
    ]
    lib.cro_lds_scrub_run_records.restype = ctypes.c_int
    _lib = lib
    return lib


def _lds_scrub_opts(lds_bytes=0, grid=0, max_rounds=0, skip_recheck=0, fill_word=0,
                    min_cu_fraction=0.0, selftest_mode=0, selftest_pattern=0, selftest_word=0,
                    selftest_bit=0) -> CroLdsScrubOpts:
    return CroLdsScrubOpts(
        lds_bytes=int(lds_bytes), grid=int(grid), max_rounds=int(max_rounds),
        skip_recheck=int(skip_recheck), fill_word=int(fill_word) & 0xFFFFFFFF,
        selftest_mode=int(selftest_mode), selftest_pattern=int(selftest_pattern) & 0xFFFFFFFF,
        selftest_word=int(selftest_word) & 0xFFFFFFFF, selftest_bit=int(selftest_bit),
        min_cu_fraction=float(min_cu_fraction),
    )


def run_lds_scrub(device: int = 0, **opts) -> dict:
    """Place one workgroup on every CU of ``device``; each counts the words of
    its LDS that differ from ``fill_word``, fills them and reads them back, and
    a further dispatch counts once more (``recheck_dirty_words``).  Options as
    ``struct CroLdsScrubOpts``; zero takes the library default.  Residue
    always fails (rc -42); the CUs reached are reported as ``cus_seen`` of
    ``cus_expected`` and gate only when ``min_cu_fraction`` > 0 (rc -43).  The
    ``selftest_*`` options are for tests."""
    lib = load_lds_scrub_library(required=True)
    c_opts = _lds_scrub_opts(**opts)
    res = CroLdsScrubResult()
    rc = lib.cro_lds_scrub_run(device, ctypes.byref(c_opts), ctypes.byref(res))
    return _result_dict(res, rc)


def run_lds_scrub_records(device: int = 0, max_records: int = 4096, **opts):
    """run_lds_scrub, and the rounds' per-workgroup records as a list of dicts
    in dispatch order (at most ``max_records``).  For tests."""
    lib = load_lds_scrub_library(required=True)
    c_opts = _lds_scrub_opts(**opts)
    res = CroLdsScrubResult()
    records = (CroLdsScrubRecord * max_records)()
    rc = lib.cro_lds_scrub_run_records(device, ctypes.byref(c_opts), ctypes.byref(res), records,
                                       max_records)
    n = min(int(res.workgroups), max_records)
    names = [name for name, _ in CroLdsScrubRecord._fields_ if name != "reserved"]
    return _result_dict(res, rc), [{k: getattr(r, k) for k in names} for r in records[:n]]
