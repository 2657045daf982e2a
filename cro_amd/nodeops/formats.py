"""ctypes wrapper for the matrix-format probe stage (cro_amd/hip/formats.hip →
libcroformats.so): exact checks of the f16, fp8, bf8, block-scaled fp8 / fp6 /
fp4 and f64 matrix paths on every CU and SIMD, with fault location, and the
numpy mirrors of what cro_amd/hip/croformats.h builds on the host: decode
tables, packers, inputs, expected tiles and the aggregation of the per-wave
records.

The loader takes ``required=False`` for callers that only ask whether the
stage is available; running the stage without the compiled library is an
error, never a silent pass.  What the stage covers and what it does not (NaN
and infinity handling, the sparse instructions, rates) is in croformats.h.
"""

from __future__ import annotations

import ctypes
import os
from typing import Optional

from .probe import (_gpu_present, _lcg_stream, _result_dict, _run_with_records,
                    aggregate_wave_records)

_LIB_PATH = os.path.join(os.path.dirname(__file__), "..", "hip", "libcroformats.so")

FORMATS_TESTS = ("mfma_f16", "mfma_fp8", "mfma_bf8", "mx_fp8", "mx_fp6", "mx_fp4", "mfma_f64")
RC_MISMATCH = -32
RC_COVERAGE = -33

# operand formats: the first five numbers are the instruction's cbsz / blgp codes
E4M3, E5M2, E2M3, E3M2, E2M1, F16, F64 = range(7)
FORMAT_BITS = (8, 8, 6, 6, 4, 16, 64)
_EBITS_MBITS_BIAS = {E4M3: (4, 3, 7), E5M2: (5, 2, 15), E2M3: (2, 3, 1), E3M2: (3, 2, 3),
                     E2M1: (2, 1, 1), F16: (5, 10, 15)}


class FormatsTest:
    """Mirror of one row of ``cro_fmt_test`` (croformats.h)."""

    def __init__(self, name, m, k, kstep, fmt_a, e_lo_a, e_n_a, fmt_b, e_lo_b, e_n_b,
                 scale_base_a, scale_base_b, scale_spread, op_sel_a, op_sel_b, lcg_salt,
                 q_a, q_b):
        self.name, self.m, self.k, self.kstep = name, m, k, kstep
        self.fmt_a, self.e_lo_a, self.e_n_a = fmt_a, e_lo_a, e_n_a
        self.fmt_b, self.e_lo_b, self.e_n_b = fmt_b, e_lo_b, e_n_b
        self.scale_base_a, self.scale_base_b = scale_base_a, scale_base_b
        self.scale_spread = scale_spread
        self.op_sel_a, self.op_sel_b = op_sel_a, op_sel_b
        self.lcg_salt = lcg_salt
        self.q_a, self.q_b = q_a, q_b  # common quantum of each side's code set

    @property
    def scaled(self) -> bool:
        return self.scale_base_a != 0

    @property
    def elems(self) -> int:
        return self.m * self.m


FORMATS_TABLE = (
    FormatsTest("mfma_f16", 16, 64, 32, F16, 0, 0, F16, 0, 0, 0, 0, 0, 0, 0, 0x27D4EB2F,
                2.0 ** -4, 2.0 ** -4),
    FormatsTest("mfma_fp8", 16, 64, 32, E4M3, 7, 3, E4M3, 7, 3, 0, 0, 0, 0, 0, 0x165667B1,
                2.0 ** -3, 2.0 ** -3),
    FormatsTest("mfma_bf8", 32, 32, 16, E5M2, 14, 4, E5M2, 14, 4, 0, 0, 0, 0, 0, 0xD3A2646C,
                2.0 ** -3, 2.0 ** -3),
    FormatsTest("mx_fp8", 16, 256, 128, E4M3, 7, 3, E5M2, 15, 3, 120, 134, 1, 1, 2, 0xFD7046C5,
                2.0 ** -3, 2.0 ** -2),
    FormatsTest("mx_fp6", 32, 128, 64, E2M3, 0, 4, E3M2, 2, 4, 120, 134, 1, 0, 0, 0xB55A4F09,
                2.0 ** -3, 2.0 ** -3),
    FormatsTest("mx_fp4", 16, 256, 128, E2M1, 0, 4, E2M1, 0, 4, 120, 134, 2, 3, 1, 0x2545F491,
                2.0 ** -1, 2.0 ** -1),
    FormatsTest("mfma_f64", 16, 64, 4, F64, 0, 0, F64, 0, 0, 0, 0, 0, 0, 0, 0x9E3779B1,
                1.0, 1.0),
)


def _test_index(test) -> int:
    return FORMATS_TESTS.index(test) if isinstance(test, str) else int(test)


class CroFormatsOpts(ctypes.Structure):
    """Mirror of ``struct CroFormatsOpts`` (cro_amd/hip/croformats.h)."""

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


class CroFormatsRecord(ctypes.Structure):
    """Mirror of ``struct CroFormatsRecord`` (cro_amd/hip/croformats.h)."""

    _fields_ = [(name, ctypes.c_uint) for name in (
        "xcc_id", "hw_id", "fail_mask", "n_bad", "first_bad", "bits_bad", "valid", "reserved")]


# fields of the nested ``struct CroFormatsAgg`` (croformats.h), in order
FORMATS_AGG_FIELDS = (
    [("waves_run", ctypes.c_ulonglong), ("waves_bad", ctypes.c_ulonglong)]
    + [(f"bad_{name}", ctypes.c_ulonglong) for name in FORMATS_TESTS]
    + [("first_bad_index", ctypes.c_longlong)]
    + [(n, ctypes.c_int) for n in
       ("cus_seen", "xcds_seen", "simds_seen", "cus_bad", "xcd", "se", "sh", "cu", "simd")]
    + [(n, ctypes.c_uint) for n in
       ("first_fail_mask", "n_bad", "first_bad", "bits_bad", "reserved")]
)


class CroFormatsResult(ctypes.Structure):
    """Mirror of ``struct CroFormatsResult`` (cro_amd/hip/croformats.h), with
    the nested aggregate's fields written out flat."""

    _fields_ = (
        [
            ("ok", ctypes.c_int),
            ("rc", ctypes.c_int),
            ("cus_expected", ctypes.c_int),
            ("rounds", ctypes.c_int),
        ]
        + FORMATS_AGG_FIELDS
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


def load_formats_library(required: Optional[bool] = None) -> Optional[ctypes.CDLL]:
    """Load libcroformats.so.  required=None → required iff a GPU is present;
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
                f"libcroformats.so missing at {path} — build it with "
                "`python -m cro_amd.hip.build` (hipcc --offload-arch=gfx950)"
            )
        return None
    lib = ctypes.CDLL(path)
    lib.cro_formats_run.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroFormatsOpts), ctypes.POINTER(CroFormatsResult),
    ]
    lib.cro_formats_run.restype = ctypes.c_int
    lib.cro_formats_run_records.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroFormatsOpts), ctypes.POINTER(CroFormatsResult),
        ctypes.POINTER(CroFormatsRecord), ctypes.c_int,
    ]
    lib.cro_formats_run_records.restype = ctypes.c_int
    lib.cro_formats_tile.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
    ]
    lib.cro_formats_tile.restype = ctypes.c_int
    _lib = lib
    return lib


def _formats_opts(grid_blocks=0, iters=0, max_rounds=0, seed=0, min_cu_fraction=0.0,
                  selftest_mode=0, selftest_test=0, selftest_elem=0, selftest_bit=0,
                  selftest_key=0, selftest_also=None) -> CroFormatsOpts:
    return CroFormatsOpts(
        grid_blocks=int(grid_blocks), iters=int(iters), max_rounds=int(max_rounds),
        seed=int(seed) & 0xFFFFFFFF, selftest_mode=int(selftest_mode),
        selftest_test=_test_index(selftest_test), selftest_bit=int(selftest_bit),
        selftest_elem=int(selftest_elem), selftest_key=int(selftest_key),
        selftest_also=0 if selftest_also is None else 1 + _test_index(selftest_also),
        min_cu_fraction=float(min_cu_fraction),
    )


def run_formats(device: int = 0, **opts) -> dict:
    """Matrix-format stage: the seven exact matrix checks of croformats.h on
    every CU and SIMD, with the location of the first bad wave.  Options as
    ``struct CroFormatsOpts``; zero takes the library default.  A data mismatch
    always fails (rc -32); coverage is reported and gates only when
    ``min_cu_fraction`` > 0 (rc -33).  The ``selftest_*`` options are for
    tests."""
    lib = load_formats_library(required=True)
    c_opts = _formats_opts(**opts)
    res = CroFormatsResult()
    rc = lib.cro_formats_run(device, ctypes.byref(c_opts), ctypes.byref(res))
    return _result_dict(res, rc)


def run_formats_records(device: int = 0, **opts):
    """As run_formats, and returns the raw per-wave records as well: a
    structured numpy array of rounds * grid_blocks * 4 records, round-major."""
    lib = load_formats_library(required=True)
    c_opts = _formats_opts(**opts)
    res = CroFormatsResult()
    return _run_with_records(CroFormatsRecord, c_opts, res, lambda buf, cap: (
        lib.cro_formats_run_records(device, ctypes.byref(c_opts), ctypes.byref(res), buf, cap)))


# -- numpy mirrors of croformats.h ---------------------------------------------------


def decode_table(fmt: int):
    """All codes of a narrow format (or of f16) as float64: cro_fmt_decode."""
    import numpy as np

    ebits, mbits, bias = _EBITS_MBITS_BIAS[fmt]
    code = np.arange(1 << FORMAT_BITS[fmt], dtype=np.int64)
    sign = (code >> (ebits + mbits)) & 1
    e = (code >> mbits) & ((1 << ebits) - 1)
    m = code & ((1 << mbits) - 1)
    mag = np.where(e > 0, np.ldexp(((1 << mbits) + m).astype(np.float64), e - bias - mbits),
                   np.ldexp(m.astype(np.float64), 1 - bias - mbits))
    if fmt == E4M3:
        mag = np.where((code & 0x7F) == 0x7F, np.nan, mag)
    elif fmt in (E5M2, F16):
        top = e == (1 << ebits) - 1
        mag = np.where(top, np.where(m != 0, np.nan, np.inf), mag)
    return np.where(sign == 1, -mag, mag)


def scale_value(e):
    """E8M0: 2^(e-127); 0xFF is NaN.  int or numpy array."""
    import numpy as np

    e = np.asarray(e, dtype=np.int64)
    return np.where(e == 0xFF, np.nan, np.ldexp(1.0, e - 127))


def row_bytes(fmt: int, k: int) -> int:
    return k * FORMAT_BITS[fmt] // 8


def pack_codes(fmt: int, codes):
    """Codes (any shape, last axis K) packed little-endian along the bit
    string of each row: cro_fmt_pack.  Returns uint8, last axis K * bits / 8."""
    import numpy as np

    bits = FORMAT_BITS[fmt]
    codes = np.asarray(codes, dtype=np.uint16)
    shifts = np.arange(bits, dtype=np.uint16)
    bitstr = ((codes[..., None] >> shifts) & 1).astype(np.uint8)
    bitstr = bitstr.reshape(*codes.shape[:-1], codes.shape[-1] * bits)
    return np.packbits(bitstr, axis=-1, bitorder="little")


def unpack_codes(fmt: int, packed, k: int):
    """Inverse of pack_codes: uint16 codes, last axis ``k``."""
    import numpy as np

    bits = FORMAT_BITS[fmt]
    packed = np.asarray(packed, dtype=np.uint8)
    bitstr = np.unpackbits(packed, axis=-1, bitorder="little")[..., : k * bits]
    bitstr = bitstr.reshape(*packed.shape[:-1], k, bits).astype(np.uint16)
    return (bitstr << np.arange(bits, dtype=np.uint16)).sum(axis=-1).astype(np.uint16)


def f16_of_sixteenths(m):
    """f16 bit patterns of m / 16, |m| <= 255 (cro_fmt_f16_of_sixteenths)."""
    import numpy as np

    return (np.asarray(m, dtype=np.float64) / 16.0).astype(np.float16).view(np.uint16)


def _draw_operand(t: FormatsTest, fmt, e_lo, e_n, raw):
    import numpy as np

    raw = raw.astype(np.int64)
    sign = raw >> 31
    if fmt == F16:
        mag = (raw >> 8) & 0xFF
        m = np.where(sign == 1, -mag, mag)
        return f16_of_sixteenths(m), m / 16.0
    if fmt == F64:
        mag = ((raw >> 8) & 0xFFFFF).astype(np.float64)
        return np.zeros(raw.size, dtype=np.uint16), np.where(sign == 1, -mag, mag)
    ebits, mbits, _ = _EBITS_MBITS_BIAS[fmt]
    mant = (raw >> 28) & ((1 << mbits) - 1)
    e = e_lo + ((raw >> 8) & 0xFFFF) % e_n
    codes = ((sign << (ebits + mbits)) | (e << mbits) | mant).astype(np.uint16)
    return codes, decode_table(fmt)[codes]


def formats_inputs(test, seed: int = 0) -> dict:
    """numpy mirror of cro_fmt_make: one check's codes and values (M x K),
    packed operands (M x row bytes, uint8; float64 M x K for mfma_f64) and
    scale bytes (M x K/32; all 127 where the check has none)."""
    import numpy as np

    t = FORMATS_TABLE[_test_index(test)]
    n, ns = t.m * t.k, t.m * (t.k // 32)
    raw, state = _lcg_stream((t.lcg_salt ^ seed) & 0xFFFFFFFF, n)
    codes_a, val_a = _draw_operand(t, t.fmt_a, t.e_lo_a, t.e_n_a, raw)
    raw, state = _lcg_stream(state, n)
    codes_b, val_b = _draw_operand(t, t.fmt_b, t.e_lo_b, t.e_n_b, raw)
    if t.scaled:
        width = 2 * t.scale_spread + 1
        raw, state = _lcg_stream(state, ns)
        sa = (t.scale_base_a - t.scale_spread + (raw >> np.uint32(24)) % width).astype(np.uint8)
        raw, state = _lcg_stream(state, ns)
        sb = (t.scale_base_b - t.scale_spread + (raw >> np.uint32(24)) % width).astype(np.uint8)
    else:
        sa = np.full(ns, 127, dtype=np.uint8)
        sb = np.full(ns, 127, dtype=np.uint8)
    shape = (t.m, t.k)
    out = {
        "codes_a": codes_a.reshape(shape), "codes_b": codes_b.reshape(shape),
        "val_a": val_a.reshape(shape).astype(np.float64),
        "val_b": val_b.reshape(shape).astype(np.float64),
        "scale_a": sa.reshape(t.m, t.k // 32), "scale_b": sb.reshape(t.m, t.k // 32),
    }
    if t.fmt_a == F64:
        out["packed_a"], out["packed_b"] = out["val_a"].copy(), out["val_b"].copy()
    else:
        out["packed_a"] = pack_codes(t.fmt_a, out["codes_a"])
        out["packed_b"] = pack_codes(t.fmt_b, out["codes_b"])
    return out


def formats_product(val_a, val_b, scale_a=None, scale_b=None):
    """The stage's logical product in float64 (cro_fmt_product):
    D[r][c] = sum_g 2^(sa[r][g]-127) 2^(sb[c][g]-127) sum_{k in block g} A[r][k] B[c][k];
    A and B are M x K, K-contiguous; without scales a plain A @ B.T."""
    import numpy as np

    a = np.asarray(val_a, dtype=np.float64)
    b = np.asarray(val_b, dtype=np.float64)
    if scale_a is None:
        return a @ b.T
    m, k = a.shape
    g = k // 32
    wa = scale_value(scale_a).reshape(m, g)
    wb = scale_value(scale_b).reshape(b.shape[0], g)
    part = np.einsum("rgk,cgk->rcg", a.reshape(m, g, 32), b.reshape(b.shape[0], g, 32))
    return (part * wa[:, None, :] * wb[None, :, :]).sum(axis=2)


def formats_expected(test, seed: int = 0):
    """numpy mirror of cro_fmt_expected: the expected tile as float32 (float64
    for mfma_f64), M x M."""
    import numpy as np

    idx = _test_index(test)
    inputs = formats_inputs(idx, seed)
    d = formats_product(inputs["val_a"], inputs["val_b"], inputs["scale_a"], inputs["scale_b"])
    return d if FORMATS_TABLE[idx].fmt_a == F64 else d.astype(np.float32)


def formats_abs_quanta(test, seed: int = 0) -> float:
    """Largest sum over k of |a b| (scale product) of any output element of the
    real inputs, in quanta q_a q_b (smallest scale product): cro_fmt_abs_quanta."""
    import numpy as np

    t = FORMATS_TABLE[_test_index(test)]
    inputs = formats_inputs(test, seed)
    total = formats_product(np.abs(inputs["val_a"]), np.abs(inputs["val_b"]),
                            inputs["scale_a"], inputs["scale_b"])
    smin = 1.0
    if t.scaled:
        smin = float(scale_value(t.scale_base_a - t.scale_spread)
                     * scale_value(t.scale_base_b - t.scale_spread))
    return float(total.max() / (t.q_a * t.q_b * smin))


def aggregate_formats_records(records) -> dict:
    """numpy mirror of cro_formats_aggregate (probe.aggregate_wave_records)."""
    return aggregate_wave_records(records, FORMATS_TESTS)[0]


def formats_test_name(fail_mask: int) -> str:
    """The lowest failing check of a fail mask (cro_fmt_test_name)."""
    for bit, name in enumerate(FORMATS_TESTS):
        if fail_mask & (1 << bit):
            return name
    return ""


# -- raw tile entry -----------------------------------------------------------------


def formats_tile(device: int, test, codes_a, codes_b, scale_a=None, scale_b=None,
                 op_sel_a: int = 0, op_sel_b: int = 0):
    """One wave of the stage's own product code for check ``test`` on caller
    data: ``codes_a`` and ``codes_b`` are M x K arrays of codes of the check's
    operand formats (float64 values for mfma_f64), K a multiple of the
    instruction's K up to 4096; ``scale_a`` / ``scale_b`` M x K/32 E8M0 bytes
    for the scaled checks.  Returns D, M x M float32 (float64 for mfma_f64)."""
    import numpy as np

    lib = load_formats_library(required=True)
    idx = _test_index(test)
    t = FORMATS_TABLE[idx]
    a = np.asarray(codes_a)
    b = np.asarray(codes_b)
    k = a.shape[1] if a.ndim == 2 else -1
    if a.shape != (t.m, k) or b.shape != (t.m, k):
        raise ValueError(f"{t.name} tile wants A and B {t.m} x K")
    if t.fmt_a == F64:
        a_dev = np.ascontiguousarray(a, dtype=np.float64)
        b_dev = np.ascontiguousarray(b, dtype=np.float64)
        d = np.zeros((t.m, t.m), dtype=np.float64)
    else:
        a_dev = np.ascontiguousarray(pack_codes(t.fmt_a, a))
        b_dev = np.ascontiguousarray(pack_codes(t.fmt_b, b))
        d = np.zeros((t.m, t.m), dtype=np.float32)
    sa = sb = None
    if t.scaled:
        sa = np.ascontiguousarray(scale_a, dtype=np.uint8)
        sb = np.ascontiguousarray(scale_b, dtype=np.uint8)
        if sa.shape != (t.m, k // 32) or sb.shape != (t.m, k // 32):
            raise ValueError(f"{t.name} tile wants scales {t.m} x K/32")
    rc = lib.cro_formats_tile(
        device, idx, int(op_sel_a), int(op_sel_b), a_dev.ctypes.data, b_dev.ctypes.data,
        sa.ctypes.data if sa is not None else None, sb.ctypes.data if sb is not None else None,
        d.ctypes.data, k,
    )
    if rc != 0:
        raise RuntimeError(f"cro_formats_tile failed: rc={rc}")
    return d
