"""ctypes wrapper for the data-movement probe stage (cro_amd/hip/movement.hip →
libcromovement.so): exact checks of the DPP crossbar, ds_swizzle / ds_permute /
ds_bpermute, v_readlane / v_readfirstlane / v_writelane, the half-wave swaps,
the transposed LDS reads and LDS-DMA on every CU and SIMD, with fault
location, and the numpy mirrors of what cro_amd/hip/cromovement.h decides on
the host: every check's and variant's source map, the payload hash, the LDS
and global images and the aggregation of the per-wave records.

The loader takes ``required=False`` for callers that only ask whether the
stage is available; running the stage without the compiled library is an
error, never a silent pass.  What the stage covers and what it does not is at
the head of cromovement.h.
"""

from __future__ import annotations

import ctypes
import os
from typing import Optional

from .probe import _gpu_present, _result_dict, _run_with_records, aggregate_wave_records

_LIB_PATH = os.path.join(os.path.dirname(__file__), "..", "hip", "libcromovement.so")

MOVEMENT_TESTS = ("dpp", "swizzle", "bpermute", "permlane_swap", "readlane",
                  "lds_tr16", "lds_tr8", "lds_tr4", "lds_tr6", "lds_dma")
DPP, SWIZZLE, BPERMUTE, PLSWAP, READLANE, TR16, TR8, TR4, TR6, DMA = range(10)
RC_MISMATCH = -36
RC_COVERAGE = -37

SRC_ZERO = -1  # source code: the destination reads 0
OLD = 64  # source code bit: source register 1 (`old`)
IMAGE_BYTES = 2048
GUARD = 32
DMA_OFFSET = 64
SRC_WORDS = 2048
POISON = 0x5EEDF00D
MASK32 = 0xFFFFFFFF

_VARIANTS = (13, 5, 3, 2, 4, 2, 2, 2, 2, 3)
VARIANT_NAMES = {
    DPP: ("quad_perm:[1,3,0,2]", "row_shl:1 bound_ctrl", "row_shr:3", "row_ror:5", "row_mirror",
          "row_half_mirror", "wave_shl:1", "wave_shr:1 bound_ctrl", "wave_rol:1", "wave_ror:1",
          "row_bcast:15 row_mask:0xa", "row_bcast:31 row_mask:0xc", "row_shr:1 bank_mask:0x5"),
    SWIZZLE: ("quad_perm:[2,0,3,1]", "swap", "reverse", "broadcast", "mixed"),
    BPERMUTE: ("pull permutation", "pull many-to-one", "push permutation"),
    PLSWAP: ("permlane16_swap", "permlane32_swap"),
    READLANE: ("readlane", "readfirstlane", "readfirstlane partial EXEC", "writelane"),
    TR16: ("stride 32", "stride 40"),
    TR8: ("stride 16", "stride 24"),
    TR4: ("row codes", "column codes"),
    TR6: ("row codes", "column codes"),
    DMA: ("dword", "dwordx4", "dword offset:64"),
}
# variants declared permutations of the wave's 64 source words of register 0
PERMUTATIONS = (
    [(DPP, v) for v in (0, 3, 4, 5, 8, 9)] + [(SWIZZLE, v) for v in (0, 1, 2)]
    + [(BPERMUTE, 0), (BPERMUTE, 2)]
)
# (ctrl, row_mask, bank_mask, bound_ctrl) of cro_mov_dpp
DPP_TABLE = (
    (0x8D, 0xF, 0xF, 0), (0x101, 0xF, 0xF, 1), (0x113, 0xF, 0xF, 0), (0x125, 0xF, 0xF, 0),
    (0x140, 0xF, 0xF, 0), (0x141, 0xF, 0xF, 0), (0x130, 0xF, 0xF, 0), (0x138, 0xF, 0xF, 1),
    (0x134, 0xF, 0xF, 0), (0x13C, 0xF, 0xF, 0), (0x142, 0xA, 0xF, 0), (0x143, 0xC, 0xF, 0),
    (0x111, 0xF, 0x5, 0),
)
SWIZZLE_TABLE = (0x8072, 0x041F, 0x7C1F, 0x00B8, 0x4917)
# bits, rows, lanes per row, bytes a lane reads: cro_mov_tr
TR_TABLE = {TR16: (16, 4, 4, 8), TR8: (8, 8, 2, 8), TR4: (4, 16, 1, 8), TR6: (6, 16, 1, 12)}
_TR_STRIDES = {TR16: (32, 40), TR8: (16, 24), TR4: (8, 16), TR6: (16, 32)}


def _test_index(test) -> int:
    return MOVEMENT_TESTS.index(test) if isinstance(test, str) else int(test)


def movement_variants(test) -> int:
    return _VARIANTS[_test_index(test)]


def movement_regs(test, variant: int) -> int:
    """Destination registers of a variant: cro_mov_regs."""
    t = _test_index(test)
    if t in (PLSWAP, TR16, TR8, TR4):
        return 2
    if t == TR6:
        return 3
    if t == DMA:
        return 5 if variant == 1 else 2
    return 1


def movement_elem(variant: int, reg: int, lane: int) -> int:
    """An element of a check as first_bad and selftest_elem hold it."""
    return (variant << 12) | (reg << 6) | lane


def decode_first_bad(first_bad: int) -> dict:
    return {"variant": (first_bad >> 12) & 0xFFFFF, "register": (first_bad >> 6) & 63,
            "lane": first_bad & 63}


class CroMovementOpts(ctypes.Structure):
    """Mirror of ``struct CroMovementOpts`` (cro_amd/hip/cromovement.h)."""

    _fields_ = [
        ("grid_blocks", ctypes.c_int),
        ("iters", ctypes.c_int),
        ("max_rounds", ctypes.c_int),
        ("seed", ctypes.c_uint),
        ("selftest_mode", ctypes.c_int),
        ("selftest_test", ctypes.c_int),
        ("selftest_bit", ctypes.c_int),
        ("selftest_elem", ctypes.c_uint),
        ("selftest_key", ctypes.c_uint),
        ("selftest_also", ctypes.c_int),
        ("min_cu_fraction", ctypes.c_double),
    ]


class CroMovementRecord(ctypes.Structure):
    """Mirror of ``struct CroMovementRecord`` (cro_amd/hip/cromovement.h)."""

    _fields_ = [(name, ctypes.c_uint) for name in (
        "xcc_id", "hw_id", "fail_mask", "n_bad", "first_bad", "bits_bad", "valid", "reserved")]


# fields of the nested ``struct CroMovementAgg`` (cromovement.h), in order
MOVEMENT_AGG_FIELDS = (
    [("waves_run", ctypes.c_ulonglong), ("waves_bad", ctypes.c_ulonglong)]
    + [(f"bad_{name}", ctypes.c_ulonglong) for name in MOVEMENT_TESTS]
    + [(n, ctypes.c_int) for n in
       ("cus_seen", "xcds_seen", "simds_seen", "cus_bad", "xcd", "se", "sh", "cu", "simd")]
    + [(n, ctypes.c_uint) for n in
       ("fail_mask", "first_fail_mask", "n_bad", "first_bad", "bits_bad")]
    + [("first_bad_index", ctypes.c_longlong)]
)


class CroMovementResult(ctypes.Structure):
    """Mirror of ``struct CroMovementResult`` (cro_amd/hip/cromovement.h), with
    the nested aggregate's fields written out flat."""

    _fields_ = (
        [
            ("ok", ctypes.c_int),
            ("rc", ctypes.c_int),
            ("cus_expected", ctypes.c_int),
            ("rounds", ctypes.c_int),
        ]
        + MOVEMENT_AGG_FIELDS
        + [
            ("first_bad_round", ctypes.c_int),
            ("first_bad_record", ctypes.c_int),
            ("grid_blocks", ctypes.c_int),
            ("iters", ctypes.c_int),
            ("gpu_ms", ctypes.c_double),
            ("t_total_ms", ctypes.c_double),
            ("failed_test", ctypes.c_char * 16),
            ("msg", ctypes.c_char * 256),
        ]
    )


_lib = None


def load_movement_library(required: Optional[bool] = None) -> Optional[ctypes.CDLL]:
    """Load libcromovement.so.  required=None → required iff a GPU is present;
    required=False → None where the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if required is None:
        required = _gpu_present()
    path = os.path.abspath(_LIB_PATH)
    if not os.path.exists(path):
        if required:
            raise RuntimeError(
                f"libcromovement.so missing at {path} — build it with "
                "`python -m cro_amd.hip.build` (hipcc --offload-arch=gfx950)"
            )
        return None
    lib = ctypes.CDLL(path)
    lib.cro_movement_run.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroMovementOpts), ctypes.POINTER(CroMovementResult),
    ]
    lib.cro_movement_run.restype = ctypes.c_int
    lib.cro_movement_run_records.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroMovementOpts), ctypes.POINTER(CroMovementResult),
        ctypes.POINTER(CroMovementRecord), ctypes.c_int,
    ]
    lib.cro_movement_run_records.restype = ctypes.c_int
    lib.cro_movement_tile.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
    ]
    lib.cro_movement_tile.restype = ctypes.c_int
    _lib = lib
    return lib


def _movement_opts(grid_blocks=0, iters=0, max_rounds=0, seed=0, min_cu_fraction=0.0,
                   selftest_mode=0, selftest_test=0, selftest_elem=0, selftest_bit=0,
                   selftest_key=0, selftest_also=None) -> CroMovementOpts:
    return CroMovementOpts(
        grid_blocks=int(grid_blocks), iters=int(iters), max_rounds=int(max_rounds),
        seed=int(seed) & MASK32, selftest_mode=int(selftest_mode),
        selftest_test=_test_index(selftest_test), selftest_bit=int(selftest_bit),
        selftest_elem=int(selftest_elem), selftest_key=int(selftest_key),
        selftest_also=0 if selftest_also is None else 1 + _test_index(selftest_also),
        min_cu_fraction=float(min_cu_fraction),
    )


def run_movement(device: int = 0, **opts) -> dict:
    """Data-movement stage: the ten exact checks of cromovement.h on every CU
    and SIMD, with the location of the first bad wave.  Options as ``struct
    CroMovementOpts``; zero takes the library default.  A data mismatch always
    fails (rc -36); coverage is reported and gates only when
    ``min_cu_fraction`` > 0 (rc -37).  The ``selftest_*`` options are for
    tests."""
    lib = load_movement_library(required=True)
    c_opts = _movement_opts(**opts)
    res = CroMovementResult()
    rc = lib.cro_movement_run(device, ctypes.byref(c_opts), ctypes.byref(res))
    return _result_dict(res, rc)


def run_movement_records(device: int = 0, **opts):
    """As run_movement, and returns the raw per-wave records as well: a
    structured numpy array of rounds * grid_blocks * 4 records, round-major."""
    lib = load_movement_library(required=True)
    c_opts = _movement_opts(**opts)
    res = CroMovementResult()
    return _run_with_records(CroMovementRecord, c_opts, res, lambda buf, cap: (
        lib.cro_movement_run_records(device, ctypes.byref(c_opts), ctypes.byref(res), buf, cap)))


def movement_tile(device: int, test, variant: int, data, addr=None):
    """One wave of the stage's own device function for ``test`` and ``variant``
    on caller data (cro_movement_tile).  ``data``: checks 0..4 a 2 x 64 uint32
    array (src, old); checks 5..8 the LDS image as bytes (uint8, a multiple of
    4, at most 2048); check 9 the global image (at most 8192 bytes).  ``addr``:
    64 ints, see cromovement.h.  Returns the raw destination registers,
    regs x 64 uint32."""
    import numpy as np

    lib = load_movement_library(required=True)
    t = _test_index(test)
    if t <= READLANE:
        buf = np.ascontiguousarray(data, dtype=np.uint32)
        if buf.shape != (2, 64):
            raise ValueError("checks 0..4 want 2 x 64 source words")
    else:
        buf = np.ascontiguousarray(data, dtype=np.uint8)
    a = None if addr is None else np.ascontiguousarray(addr, dtype=np.int32)
    if a is not None and a.shape != (64,):
        raise ValueError("addr wants 64 values")
    out = np.zeros((movement_regs(t, variant), 64), dtype=np.uint32)
    rc = lib.cro_movement_tile(device, t, int(variant), buf.ctypes.data, buf.nbytes,
                               None if a is None else a.ctypes.data, out.ctypes.data, out.nbytes)
    if rc != 0:
        raise RuntimeError(f"cro_movement_tile failed: rc={rc}")
    return out


# -- numpy mirrors of cromovement.h ---------------------------------------------------


def _lcg(s):
    import numpy as np

    return (np.asarray(s, dtype=np.uint64) * 1664525 + 1013904223) & MASK32


def movement_salt(seed: int, rep: int) -> int:
    """cro_mov_salt."""
    return int(_lcg(_lcg((seed ^ ((rep + 1) * 0x9E3779B9)) & MASK32)))


def movement_payload(salt: int, test: int, variant: int, lane, reg):
    """cro_mov_payload: the word source register ``reg`` of lane ``lane`` holds
    (lane and reg int or arrays)."""
    import numpy as np

    key = (test << 20) | (variant << 12) | (np.asarray(reg, dtype=np.uint64) << 6) \
        | np.asarray(lane, dtype=np.uint64)
    return _lcg(_lcg(np.uint64(salt) ^ key)).astype(np.uint32)


def movement_rt(seed: int, rep: int) -> dict:
    """cro_mov_rt: the run-time values of repeat ``rep``."""
    salt = movement_salt(seed, rep)
    h = int(_lcg(salt ^ 0x5BD1E995)) >> 8
    a = ((h >> 12) & 63) | 1
    if a in (1, 63):
        a = 37
    return {"salt": salt, "sel": ((int(_lcg(seed & MASK32)) >> 26) + rep) & 63,
            "fa": 1 + h % 63, "wl": (h >> 6) & 63, "a": a, "b": (h >> 18) & 63}


def inv64(a: int) -> int:
    """cro_mov_inv64."""
    x = a
    x = (x * (2 - a * x)) & MASK32
    x = (x * (2 - a * x)) & MASK32
    return x & 63


def dpp_source(variant: int):
    """cro_mov_dpp_src for the 64 lanes: source codes."""
    import numpy as np

    ctrl, row_mask, bank_mask, bound = DPP_TABLE[variant]
    out = np.zeros(64, dtype=np.int64)
    for lane in range(64):
        row, i, keep = lane >> 4, lane & 15, OLD | lane
        if not (row_mask >> row) & 1 or not (bank_mask >> (i >> 2)) & 1:
            out[lane] = keep
            continue
        n, valid = ctrl & 15, True
        if ctrl < 0x100:
            s = (lane & ~3) | ((ctrl >> (2 * (lane & 3))) & 3)
        elif ctrl < 0x110:
            valid, s = i + n < 16, lane + n
        elif ctrl < 0x120:
            valid, s = i - n >= 0, lane - n
        elif ctrl < 0x130:
            s = (lane & ~15) | ((i - n) & 15)
        elif ctrl == 0x130:
            valid, s = lane < 63, lane + 1
        elif ctrl == 0x134:
            s = (lane + 1) & 63
        elif ctrl == 0x138:
            valid, s = lane > 0, lane - 1
        elif ctrl == 0x13C:
            s = (lane - 1) & 63
        elif ctrl == 0x140:
            s = (lane & ~15) | (15 - i)
        elif ctrl == 0x141:
            s = lane ^ 7
        elif ctrl == 0x142:
            valid, s = row > 0, 16 * row - 1
        else:
            valid, s = row > 1, 31
        out[lane] = s if valid else (SRC_ZERO if bound else keep)
    return out


def dpp_keeps_old(variant: int):
    """The lanes of a dpp variant that keep ``old``, from the masks and
    bound_ctrl alone (an independent statement of the rule)."""
    import numpy as np

    ctrl, row_mask, bank_mask, bound = DPP_TABLE[variant]
    lane = np.arange(64)
    row, i = lane >> 4, lane & 15
    masked = (((row_mask >> row) & 1) == 0) | (((bank_mask >> (i >> 2)) & 1) == 0)
    n = ctrl & 15
    invalid = np.zeros(64, dtype=bool)
    if 0x101 <= ctrl <= 0x10F:
        invalid = i + n > 15
    elif 0x111 <= ctrl <= 0x11F:
        invalid = i < n
    elif ctrl == 0x130:
        invalid = lane == 63
    elif ctrl == 0x138:
        invalid = lane == 0
    elif ctrl == 0x142:
        invalid = row == 0
    elif ctrl == 0x143:
        invalid = row < 2
    return masked | (invalid & (bound == 0))


def swizzle_source(variant: int):
    """cro_mov_swizzle_src for the 64 lanes."""
    import numpy as np

    o = SWIZZLE_TABLE[variant]
    lane = np.arange(64)
    if o & 0x8000:
        return (lane & ~3) | ((o >> (2 * (lane & 3))) & 3)
    return (lane & 32) | ((((lane & 31) & (o & 31)) | ((o >> 5) & 31)) ^ ((o >> 10) & 31))


def bperm_index(variant: int, rt: dict):
    """cro_mov_bperm_idx: the lane number every lane passes."""
    import numpy as np

    lane = np.arange(64)
    return (((lane >> 1) if variant == 1 else lane) * rt["a"] + rt["b"]) & 63


def bperm_apply(variant: int, idx, src):
    """What ds_bpermute (variants 0, 1) or ds_permute (2) delivers for the
    indices ``idx`` (lane numbers): pull reads lane idx[i], push writes lane
    idx[i] (a destination nobody writes reads 0)."""
    import numpy as np

    idx = np.asarray(idx) & 63
    src = np.asarray(src, dtype=np.uint32)
    if variant != 2:
        return src[idx]
    out = np.zeros(64, dtype=np.uint32)
    out[idx] = src
    return out


def movement_source_map(test, variant: int, rt: Optional[dict] = None):
    """Source codes of checks 0..4 (cro_mov_src), regs x 64: (register << 6) |
    lane of the source word, or SRC_ZERO."""
    import numpy as np

    t = _test_index(test)
    lane = np.arange(64)
    if t == DPP:
        return dpp_source(variant)[None, :]
    if t == SWIZZLE:
        return swizzle_source(variant)[None, :]
    if t == BPERMUTE:
        if variant != 2:
            return bperm_index(variant, rt)[None, :]
        return (((lane - rt["b"]) * inv64(rt["a"])) & 63)[None, :]
    if t == PLSWAP:
        if variant == 0:
            odd = ((lane >> 4) & 1) == 1
            return np.stack([np.where(odd, OLD | (lane - 16), lane),
                             np.where(odd, OLD | lane, lane + 16)])
        low = lane < 32
        return np.stack([np.where(low, lane, OLD | (lane - 32)),
                         np.where(low, lane + 32, OLD | lane)])
    if t == READLANE:
        if variant == 0:
            return np.full((1, 64), rt["sel"])
        if variant == 1:
            return np.zeros((1, 64), dtype=np.int64)
        if variant == 2:
            return np.where(lane >= rt["fa"], rt["fa"], OLD | lane)[None, :]
        return np.where(lane == rt["wl"], OLD | lane, lane)[None, :]
    raise ValueError(f"check {MOVEMENT_TESTS[t]} has no register source map")


def apply_source_map(codes, data):
    """The destination registers a source map delivers from ``data`` (2 x 64:
    src, old)."""
    import numpy as np

    codes = np.asarray(codes)
    data = np.asarray(data, dtype=np.uint32)
    safe = np.where(codes < 0, 0, codes)
    out = data[safe >> 6, safe & 63]
    return np.where(codes < 0, np.uint32(0), out).astype(np.uint32)


def _pack(fields, bits: int, words: int):
    """Little-endian string of b-bit fields (last axis) as ``words`` uint32."""
    import numpy as np

    fields = np.asarray(fields)
    flat = fields.reshape(-1, fields.shape[-1])
    out = np.zeros((flat.shape[0], words), dtype=np.uint32)
    for i, row in enumerate(flat):
        total = sum(int(f) << (k * bits) for k, f in enumerate(row))
        out[i] = [(total >> (32 * w)) & MASK32 for w in range(words)]
    return out.reshape(fields.shape[:-1] + (words,))


def _unpack(words, bits: int, n: int):
    """The n b-bit fields of a little-endian string of uint32 (last axis)."""
    import numpy as np

    words = np.asarray(words, dtype=np.uint32)
    flat = words.reshape(-1, words.shape[-1])
    out = np.zeros((flat.shape[0], n), dtype=np.uint32)
    for i, row in enumerate(flat):
        total = sum(int(w) << (32 * k) for k, w in enumerate(row))
        out[i] = [(total >> (k * bits)) & ((1 << bits) - 1) for k in range(n)]
    return out.reshape(words.shape[:-1] + (n,))


def tr_stride(test, variant: int) -> int:
    return _TR_STRIDES[_test_index(test)][variant]


def tr_addr(test, variant: int):
    """cro_mov_tr_addr: the byte offset every lane passes."""
    import numpy as np

    t = _test_index(test)
    _, rows, per, nbytes = TR_TABLE[t]
    stride = tr_stride(t, variant)
    lane = np.arange(64)
    g, j = lane >> 4, lane & 15
    return g * rows * stride + (j // per) * stride + (j % per) * nbytes


def tr_codes(test, variant: int, salt: int):
    """cro_mov_tr_code for all of a wave's elements: block x row x col."""
    import numpy as np

    t = _test_index(test)
    bits, rows, _, _ = TR_TABLE[t]
    block, row, col = np.meshgrid(np.arange(4), np.arange(rows), np.arange(16), indexing="ij")
    if t == TR16:
        return ((block * 64 + row * 16 + col) * 0x9E35 + salt) & 0xFFFF
    if t == TR8:
        return ((row * 16 + col) * 0x9D + block * 0x35 + salt) & 0xFF
    which = col if variant else row
    if t == TR4:
        return (which ^ salt ^ (block * 5)) & 0xF
    return ((which | (block << 4)) ^ salt) & 0x3F


def tr_image(test, variant: int, salt: int):
    """The wave's LDS image as uint32 words (cro_mov_tr_image_word)."""
    import numpy as np

    t = _test_index(test)
    bits, rows, _, _ = TR_TABLE[t]
    stride = tr_stride(t, variant)
    row_words = 16 * bits // 32
    words = np.arange(4 * rows * stride // 4, dtype=np.uint32)
    image = (np.uint32(POISON) ^ words).reshape(4, rows, stride // 4)
    image[:, :, :row_words] = _pack(tr_codes(t, variant, salt), bits, row_words)
    return image.reshape(-1)


def tr_read(test, image, addr):
    """What the transposed read of ``test`` delivers: ``image`` the LDS bytes
    (or words), ``addr`` 64 byte offsets.  Per group of 16 lanes, lane P*q+p
    supplies a P-th of row q and lane i receives column i, row q in field q.
    Returns regs x 64 uint32."""
    import numpy as np

    t = _test_index(test)
    bits, rows, per, nbytes = TR_TABLE[t]
    raw = np.ascontiguousarray(image).view(np.uint8)
    addr = np.asarray(addr, dtype=np.int64)
    chunks = np.stack([raw[a:a + nbytes] for a in addr]).reshape(4, rows, per * nbytes)
    elems = _unpack(np.ascontiguousarray(chunks).view(np.uint32), bits, 16)  # group, row, col
    regs = nbytes // 4
    return _pack(elems.transpose(0, 2, 1), bits, regs).reshape(64, regs).T.copy()


def tr_want(test, variant: int, salt: int):
    """cro_mov_tr_want for the 64 lanes: regs x 64."""
    t = _test_index(test)
    bits, rows, _, nbytes = TR_TABLE[t]
    codes = tr_codes(t, variant, salt)  # block, row, col
    return _pack(codes.transpose(0, 2, 1), bits, nbytes // 4).reshape(64, nbytes // 4).T.copy()


def dma_size(variant: int) -> int:
    return 16 if variant == 1 else 4


def dma_ioff(variant: int) -> int:
    return DMA_OFFSET if variant == 2 else 0


def dma_source_words():
    """The fixed content of the device source buffer (cro_mov_dma_word)."""
    import numpy as np

    return _lcg(_lcg(np.arange(SRC_WORDS, dtype=np.uint64) ^ 0x6D6F7631)).astype(np.uint32)


def dma_addr(variant: int, wave: int, rt: dict):
    """cro_mov_dma_addr: the byte address every lane passes."""
    import numpy as np

    chunk = (np.arange(64) * rt["a"] + rt["b"] + variant) & 63
    return wave * 1024 + chunk * dma_size(variant)


def dma_region(variant: int, image, addr):
    """The LDS words of the DMA region after the transfer: GUARD poisoned
    words, the destination (the wave-uniform base + lane * size, from the
    lane's address + the instruction offset), GUARD poisoned words."""
    import numpy as np

    n = dma_size(variant) // 4
    src = np.ascontiguousarray(image).view(np.uint32)
    region = np.full(2 * GUARD + 64 * n, POISON, dtype=np.uint32)
    first = (np.asarray(addr, dtype=np.int64) + dma_ioff(variant)) // 4
    for lane in range(64):
        region[GUARD + lane * n:GUARD + (lane + 1) * n] = src[first[lane]:first[lane] + n]
    return region


def dma_read(variant: int, image, addr):
    """The read-back registers of the DMA check: data registers (word 64 r +
    lane of the destination), then the guard register (lanes 0..31 the words
    before the destination, 32..63 those after)."""
    import numpy as np

    n = dma_size(variant) // 4
    region = dma_region(variant, image, addr)
    data = region[GUARD:GUARD + 64 * n].reshape(n, 64)
    guard = np.concatenate([region[:GUARD], region[GUARD + 64 * n:]])
    return np.concatenate([data, guard[None, :]])


def movement_expected(test, variant: int, seed: int = 0, rep: int = 0, wave: int = 0):
    """What the stage's lanes must receive in repeat ``rep``: regs x 64 uint32."""
    import numpy as np

    t = _test_index(test)
    rt = movement_rt(seed, rep)
    if t <= READLANE:
        codes = movement_source_map(t, variant, rt)
        safe = np.where(codes < 0, 0, codes)
        words = movement_payload(rt["salt"], t, variant, safe & 63, safe >> 6)
        return np.where(codes < 0, np.uint32(0), words).astype(np.uint32)
    if t <= TR6:
        return tr_want(t, variant, rt["salt"])
    return dma_read(variant, dma_source_words(), dma_addr(variant, wave, rt))


def aggregate_movement_records(records) -> dict:
    """numpy mirror of cro_movement_aggregate: probe.aggregate_wave_records
    and the OR of the fail masks."""
    out, fail_mask, _ = aggregate_wave_records(records, MOVEMENT_TESTS)
    out["fail_mask"] = fail_mask
    return out


def movement_test_name(fail_mask: int) -> str:
    """The lowest failing check of a fail mask (cro_mov_test_name)."""
    for bit, name in enumerate(MOVEMENT_TESTS):
        if fail_mask & (1 << bit):
            return name
    return ""


def describe_first_bad(test, first_bad: int) -> str:
    """"variant 3 (row_ror:5) register 0 lane 17" for a failure of ``test``."""
    d = decode_first_bad(first_bad)
    names = VARIANT_NAMES.get(_test_index(test), ()) if test != "" else ()
    label = f" ({names[d['variant']]})" if d["variant"] < len(names) else ""
    return f"variant {d['variant']}{label} register {d['register']} lane {d['lane']}"
