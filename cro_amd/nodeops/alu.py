"""ctypes wrapper for the ALU probe stage (cro_amd/hip/alu.hip → libcroalu.so):
exact checks of the vector and scalar ALUs on every CU and SIMD, with fault
location and a consensus check of the transcendental unit, and the second,
independent statement of everything cro_amd/hip/croalu.h decides on the host:
the form list, every form's operand rows and its reference (numpy / pure
Python here, C++ there; a test shows the two agree bit for bit), and the
aggregation of the per-wave records with the digest majority.

The loader takes ``required=False`` for callers that only ask whether the
stage is available; running the stage without the compiled library is an
error, never a silent pass.  What the stage covers and what it does not is at
the head of croalu.h and in docs/architecture.md.
"""

from __future__ import annotations

import ctypes
import math
import os
import struct
from collections import Counter
from typing import Optional

from .probe import _gpu_present, _result_dict, _run_with_records, aggregate_wave_records

_LIB_PATH = os.path.join(os.path.dirname(__file__), "..", "hip", "libcroalu.so")

ALU_TESTS = ("int_arith", "bit_ops", "pk_int", "dot", "f32", "f16", "f64", "convert",
             "scale_convert", "compare_select", "salu", "transcendental")
(INT, BIT, PKINT, DOT, F32, F16, F64, CVT, SCALE, CMP, SALU, TRANS) = range(12)
RC_MISMATCH = -38
RC_COVERAGE = -39
ROWS = 64
ANCHORS = 16
FMA_LO, FMA_HI = -5, 26  # bound on e(a) + e(b) - e(c) of an fma row
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF

# source words and result words of a signature (CRO_ALU_SIGS)
SIGS = {
    "V1_V": (1, 1), "V1_VV": (2, 1), "V1_VVV": (3, 1), "V1_VVO": (3, 1),
    "V1_VVVO": (4, 1), "V1_MBCNT": (3, 1), "V2_D": (2, 2), "V2_DD": (4, 2), "V2_DDD": (6, 2), "V2_VD": (3, 2),
    "V2_DV": (3, 2), "V2_VVD": (4, 2), "V2_V": (1, 2), "V2_VV": (2, 2), "V1_D": (2, 1),
    "V1_DD": (4, 1), "V1_DV": (3, 1), "V2C_VVVV": (4, 2), "V1_CMPX": (3, 1), "X_DIV": (4, 2),
    "X_SQRT": (2, 2), "V2_FP6": (6, 2), "S1_S": (1, 1), "S1_SS": (2, 1), "S1_SSSS": (4, 1), "S1C_S": (1, 2),
    "S1C_SS": (2, 2), "S2_Q": (2, 2), "S2_QQ": (4, 2), "S2_QS": (3, 2), "S1_Q": (2, 1),
    "S1C_Q": (2, 2), "S2C_SSSS": (4, 2), "SC_QQ": (4, 1), "SC_QS": (3, 1), "SC_SSSS": (4, 1),
}


# -- bit casts and roundings ---------------------------------------------------------


def f32(u: int) -> float:
    return struct.unpack("<f", struct.pack("<I", u & M32))[0]


def u32_of(x: float) -> int:
    """One nearest-even rounding of a double to f32, as bits."""
    import numpy as np

    with np.errstate(over="ignore", under="ignore"):
        return int(np.asarray(x, dtype=np.float64).astype(np.float32).view(np.uint32))


def f64(lo: int, hi: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", ((hi & M32) << 32) | (lo & M32)))[0]


def u64_of(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def half(code: int) -> float:
    import numpy as np

    return float(np.array([code & 0xFFFF], dtype=np.uint16).view(np.float16)[0])


def half_of(x: float, rtz: bool = False) -> int:
    """One rounding of a double to a half: nearest-even, or toward zero."""
    import numpy as np

    if not rtz:
        with np.errstate(over="ignore", under="ignore"):
            return int(np.asarray(x, dtype=np.float64).astype(np.float16).view(np.uint16))
    sign = 0x8000 if math.copysign(1.0, x) < 0 else 0
    a = abs(x)
    if a == 0.0:
        return sign
    if math.isinf(a):
        return sign | 0x7C00
    q = max(math.frexp(a)[1] - 1 - 10, -24)
    r = min(math.ldexp(math.floor(math.ldexp(a, -q)), q), 65504.0)
    if r == 0.0:
        return sign
    e = math.frexp(r)[1] - 1
    if e < -14:
        return sign | int(math.ldexp(r, 24))
    return sign | ((e + 15) << 10) | (int(math.ldexp(r, 10 - e)) & 0x3FF)


def bf16_of(u: int) -> int:
    return ((u + 0x7FFF + ((u >> 16) & 1)) & M32) >> 16


def bf16(code: int) -> float:
    return f32((code & 0xFFFF) << 16)


def _lcg(s: int) -> int:
    return (s * 1664525 + 1013904223) & M32


def alu_rand(seed: int, form: int, row: int, k: int) -> int:
    """cro_alu_rand."""
    x = (seed ^ 0xA10C0DE ^ ((((form * 64 + row) * 8 + k) * 0x9E3779B9) & M32)) & M32
    x = _lcg(_lcg(x))
    x ^= x >> 15
    x = _lcg(x)
    return x ^ (x >> 13)


def _sx(v: int, bits: int) -> int:
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _clz(v: int) -> int:
    return 32 - v.bit_length()


def _ctz(v: int) -> int:
    return (v & -v).bit_length() - 1


def _rev(v: int) -> int:
    return int(f"{v:032b}"[::-1], 2)


def _sat(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def _pop(v: int) -> int:
    return bin(v).count("1")


# -- references ------------------------------------------------------------------------
# name → f(s) with s the six source words; returns one word or (word0, word1).


def _f32op(fn):
    """An f32 operation of numpy's own (one IEEE rounding), on bits."""
    import numpy as np

    def run(*bits):
        with np.errstate(all="ignore"):
            args = [np.array([b], dtype=np.uint32).view(np.float32)[0] for b in bits]
            return int(np.asarray(fn(*args), dtype=np.float32).view(np.uint32))
    return run


def _fmin(x, y):  # -0 below +0
    return x if x < y else y if y < x else x if math.copysign(1.0, x) < 0 else y


def _fmax(x, y):
    return x if x > y else y if y > x else y if math.copysign(1.0, x) < 0 else x


def _halves(fn):
    def run(s):
        out = 0
        for h in (0, 16):
            out |= (fn((s[0] >> h) & 0xFFFF, (s[1] >> h) & 0xFFFF, (s[2] >> h) & 0xFFFF)
                    & 0xFFFF) << h
        return out
    return run


def _fhalves(fn):
    return _halves(lambda x, y, z: half_of(fn(half(x), half(y), half(z))))


def _A(s):
    return (s[1] << 32) | s[0]


def _B(s):
    return (s[3] << 32) | s[2]


def _w64(v: int):
    return (v & M32, (v >> 32) & M32)


def _wd(x: float):
    return _w64(u64_of(x))


def _bitop3(a, b, c, tt):
    r = 0
    for i in range(32):
        idx = (((a >> i) & 1) << 2) | (((b >> i) & 1) << 1) | ((c >> i) & 1)
        r |= ((tt >> idx) & 1) << i
    return r


def _perm(s):
    data = (s[0] << 32) | s[1]
    r = 0
    for i in range(4):
        sel = (s[2] >> (8 * i)) & 255
        if sel >= 13:
            v = 0xFF
        elif sel == 12:
            v = 0
        elif sel >= 8:
            v = 0xFF if (data >> (16 * (sel - 8) + 15)) & 1 else 0
        else:
            v = (data >> (8 * sel)) & 255
        r |= v << (8 * i)
    return r


def _bfe_i32(s):
    o, n = s[1] & 31, s[2] & 31
    if not n:
        return 0
    if o + n < 32:
        return _sx(s[0] >> o, n) & M32
    return (_sx(s[0], 32) >> o) & M32


def _dot(s, n, bits, signed):
    r = s[2]
    for i in range(n):
        x, y = s[0] >> (bits * i), s[1] >> (bits * i)
        if signed:
            r += _sx(x, bits) * _sx(y, bits)
        else:
            r += (x & ((1 << bits) - 1)) * (y & ((1 << bits) - 1))
    return r & M32


def _cvt_int(x: float, lo: int, hi: int) -> int:
    if x != x:
        return 0
    if math.isinf(x):
        return (hi if x > 0 else lo) & M32
    return _sat(int(x), lo, hi) & M32  # int() truncates


def _cvt_pk_u8(s):
    import numpy as np

    x, sh = f32(s[0]), 8 * (s[1] & 3)
    keep = s[2] & ~(255 << sh) & M32
    if x != x:
        return keep
    return keep | (_sat(int(np.rint(min(max(x, -1e6), 1e6))), 0, 255) << sh)


def _bfe64(v, sel, sign):
    o, n = sel & 63, (sel >> 16) & 127
    if not n:
        return 0
    if o + n >= 64:
        return (_sx(v, 64) >> o) & M64 if sign else v >> o
    field = (v >> o) & ((1 << n) - 1)
    return _sx(field, n) & M64 if sign else field


def _s_bfe_i32(s):
    o, n = s[1] & 31, (s[1] >> 16) & 127
    if not n:
        r = 0
    elif o + n < 32:
        r = _sx(s[0] >> o, n) & M32
    else:
        r = (_sx(s[0], 32) >> o) & M32
    return (r, int(r != 0))


def _fract(s):
    x = f32(s[0])
    r = u32_of(x - float(math.floor(x)) if x != 0 else 0.0)
    return 0x3F7FFFFF if f32(r) >= 1.0 else r


def _div_f64(s):
    import numpy as np

    with np.errstate(all="ignore"):  # IEEE divide, overflow to infinity included
        return _wd(float(np.float64(f64(s[0], s[1])) / np.float64(f64(s[2], s[3]))))


def _ldexp(x: float, n: int) -> float:
    try:
        return math.ldexp(x, n)
    except OverflowError:
        return math.copysign(math.inf, x)


def _frexp_exp(s):
    x = f32(s[0])
    return 0 if x == 0 else math.frexp(x)[1] & M32


def _clamp01(s):
    p = f32(_f32op(lambda a, b: a * b)(s[0], s[1]))
    return 0 if p <= 0 else 0x3F800000 if p > 1 else u32_of(p)


_tables = {}


def _table(fmt):
    from .formats import decode_table

    if fmt not in _tables:
        _tables[fmt] = [float(v) for v in decode_table(fmt)]
    return _tables[fmt]


_FMT_BITS = {0: 8, 1: 8, 4: 4}


def _dec(fmt, code, scale_bits):
    return u32_of(_table(fmt)[code] * f32(scale_bits))


_MINIFLOAT = {0: (4, 3, 7), 1: (5, 2, 15), 4: (2, 1, 1)}


def _plain_table(fmt):
    """The codes of a format read as plain minifloats, no specials."""
    if ("plain", fmt) not in _tables:
        ebits, mbits, bias = _MINIFLOAT[fmt]
        vals = []
        for code in range(1 << (ebits + mbits)):
            e, m = code >> mbits, code & ((1 << mbits) - 1)
            vals.append(math.ldexp((1 << mbits) + m, e - bias - mbits) if e
                        else math.ldexp(m, 1 - bias - mbits))
        _tables[("plain", fmt)] = vals
    return _tables[("plain", fmt)]


def _enc(fmt, x_bits, scale_bits, max_code):
    return _encd(fmt, f32(x_bits), scale_bits, max_code)


def _encd(fmt, x, scale_bits, max_code):
    """The nearest plain-minifloat code (ties to the even code) of x / scale,
    saturating at ``max_code``: cro_alu_encd."""
    v = abs(x / f32(scale_bits))
    x_bits = 0x80000000 if math.copysign(1.0, x) < 0 else 0
    table = _plain_table(fmt)
    best = 0
    for k in range(max_code + 1):
        dk, db = abs(table[k] - v), abs(table[best] - v)
        if dk < db or (dk == db and not k & 1):
            best = k
    return ((x_bits >> 31) << (_FMT_BITS[fmt] - 1)) | best


def _fp6_fold(s, scale_bits):
    """The 32 results of the 6-bit conversion (element i is bits 6i+5..6i of
    the 192-bit operand), folded as the stage folds them: rotate-left-5 and
    xor over the even and over the odd ones."""
    data = sum(w << (32 * k) for k, w in enumerate(s[:6]))
    w = [0, 0]
    for i in range(32):
        v = _dec(2, (data >> (6 * i)) & 63, scale_bits)
        w[i & 1] = (((w[i & 1] << 5) | (w[i & 1] >> 27)) & M32) ^ v
    return (w[0], w[1])


def _rel(x, y):
    return 8 if x != x or y != y else 1 if x < y else 2 if x == y else 4


_PRED = {"lt": 1, "eq": 2, "le": 3, "gt": 4, "lg": 5, "ne": 13, "ge": 6, "o": 7, "u": 8,
         "nge": 9, "nlt": 14}


def _class(bits, ebits, mbits):
    m = bits & ((1 << mbits) - 1)
    ex = (bits >> mbits) & ((1 << ebits) - 1)
    neg = (bits >> (ebits + mbits)) & 1
    if ex == (1 << ebits) - 1:
        return (1 if m >> (mbits - 1) else 0) if m else (2 if neg else 9)
    if ex:
        return 3 if neg else 8
    if m:
        return 4 if neg else 7
    return 5 if neg else 6


def _scc(fn):
    def run(s):
        r = fn(s) & M32
        return (r, int(r != 0))
    return run


def _s_bfe_u32(s):
    o, n = s[1] & 31, (s[1] >> 16) & 127
    r = 0 if not n else s[0] >> o if n >= 32 else (s[0] >> o) & ((1 << n) - 1)
    return (r, int(r != 0))


def _lshl_add(n):
    def run(s):
        t = (s[0] << n) + s[1]
        return (t & M32, int(t >> 32 != 0))
    return run


def _flbit_i32(a):
    if a in (0, M32):
        return M32
    return _clz(a ^ M32 if a >> 31 else a)


def _exact_t(fn):
    """A transcendental's anchor value; the other rows' expected words are
    never compared, any finite word will do for them."""
    def run(x):
        try:
            return fn(x)
        except (ValueError, ZeroDivisionError, OverflowError):
            return float("nan")
    return run


def _sinrev(x):
    """sin of x revolutions; exact at the multiples of a quarter."""
    q = 4.0 * x
    if q == math.floor(q):
        return (0.0, 1.0, 0.0, -1.0)[int(q) % 4]
    return math.sin(6.283185307179586 * x)


def _cosrev(x):
    return _sinrev(x + 0.25)


def _build_forms():
    add, sub, mul = (_f32op(lambda a, b: a + b), _f32op(lambda a, b: a - b),
                     _f32op(lambda a, b: a * b))
    import numpy as np

    F = []  # (check, name, mnemonic, signature, class, reference)

    def X(check, name, mnem, sig, cls, ref):
        F.append((check, name, mnem, sig, cls, ref))

    # int_arith
    X(INT, "add_u64", "v_addc_co_u32", "V2C_VVVV", "INT", lambda s: _w64((_A(s) + _B(s)) & M64))
    X(INT, "sub_u64", "v_subb_co_u32", "V2C_VVVV", "INT", lambda s: _w64((_A(s) - _B(s)) & M64))
    X(INT, "mul_lo_u32", "v_mul_lo_u32", "V1_VV", "INT", lambda s: (s[0] * s[1]) & M32)
    X(INT, "mul_hi_u32", "v_mul_hi_u32", "V1_VV", "INT", lambda s: (s[0] * s[1]) >> 32)
    X(INT, "mul_hi_i32", "v_mul_hi_i32", "V1_VV", "INT",
      lambda s: ((_sx(s[0], 32) * _sx(s[1], 32)) >> 32) & M32)
    X(INT, "mad_u64_u32", "v_mad_u64_u32", "V2_VVD", "INT",
      lambda s: _w64((s[0] * s[1] + _B(s)) & M64))
    X(INT, "mad_i64_i32", "v_mad_i64_i32", "V2_VVD", "INT",
      lambda s: _w64((_sx(s[0], 32) * _sx(s[1], 32) + _B(s)) & M64))
    X(INT, "mad_u32_u24", "v_mad_u32_u24", "V1_VVV", "INT",
      lambda s: ((s[0] & 0xFFFFFF) * (s[1] & 0xFFFFFF) + s[2]) & M32)
    X(INT, "mul_i32_i24", "v_mul_i32_i24", "V1_VV", "INT",
      lambda s: (_sx(s[0], 24) * _sx(s[1], 24)) & M32)
    X(INT, "lshl_add_u32", "v_lshl_add_u32", "V1_VVV", "INT",
      lambda s: ((s[0] << (s[1] & 31)) + s[2]) & M32)
    X(INT, "add3_u32", "v_add3_u32", "V1_VVV", "INT", lambda s: (s[0] + s[1] + s[2]) & M32)
    X(INT, "sad_u8", "v_sad_u8", "V1_VVV", "INT", lambda s: (s[2] + sum(
        abs(((s[0] >> i) & 255) - ((s[1] >> i) & 255)) for i in (0, 8, 16, 24))) & M32)
    # bit_ops
    v64 = lambda s: (s[2] << 32) | s[1]  # noqa: E731
    X(BIT, "lshlrev_b32", "v_lshlrev_b32", "V1_VV", "INT", lambda s: (s[1] << (s[0] & 31)) & M32)
    X(BIT, "lshrrev_b32", "v_lshrrev_b32", "V1_VV", "INT", lambda s: s[1] >> (s[0] & 31))
    X(BIT, "ashrrev_i32", "v_ashrrev_i32", "V1_VV", "INT",
      lambda s: (_sx(s[1], 32) >> (s[0] & 31)) & M32)
    X(BIT, "lshlrev_b64", "v_lshlrev_b64", "V2_VD", "INT",
      lambda s: _w64((v64(s) << (s[0] & 63)) & M64))
    X(BIT, "lshrrev_b64", "v_lshrrev_b64", "V2_VD", "INT", lambda s: _w64(v64(s) >> (s[0] & 63)))
    X(BIT, "ashrrev_i64", "v_ashrrev_i64", "V2_VD", "INT",
      lambda s: _w64((_sx(v64(s), 64) >> (s[0] & 63)) & M64))
    X(BIT, "bfe_u32", "v_bfe_u32", "V1_VVV", "INT",
      lambda s: (s[0] >> (s[1] & 31)) & ((1 << (s[2] & 31)) - 1))
    X(BIT, "bfe_i32", "v_bfe_i32", "V1_VVV", "INT", _bfe_i32)
    X(BIT, "bfi_b32", "v_bfi_b32", "V1_VVV", "INT",
      lambda s: (s[0] & s[1]) | ((s[0] ^ M32) & s[2]))
    X(BIT, "alignbit_b32", "v_alignbit_b32", "V1_VVV", "INT",
      lambda s: (((s[0] << 32) | s[1]) >> (s[2] & 31)) & M32)
    X(BIT, "alignbyte_b32", "v_alignbyte_b32", "V1_VVV", "INT",
      lambda s: (((s[0] << 32) | s[1]) >> (8 * (s[2] & 3))) & M32)
    X(BIT, "perm_b32", "v_perm_b32", "V1_VVV", "PERM", _perm)
    for tt in (0x96, 0xE8, 0xCA, 0x1B):
        X(BIT, f"bitop3_{tt:02x}", "v_bitop3_b32", "V1_VVV", "INT",
          lambda s, tt=tt: _bitop3(s[0], s[1], s[2], tt))
    X(BIT, "bfrev_b32", "v_bfrev_b32", "V1_V", "INT", lambda s: _rev(s[0]))
    X(BIT, "ffbh_u32", "v_ffbh_u32", "V1_V", "INT", lambda s: _clz(s[0]) if s[0] else M32)
    X(BIT, "ffbl_b32", "v_ffbl_b32", "V1_V", "INT", lambda s: _ctz(s[0]) if s[0] else M32)
    X(BIT, "bcnt_u32_b32", "v_bcnt_u32_b32", "V1_VV", "INT", lambda s: (_pop(s[0]) + s[1]) & M32)
    # the table holds mbcnt for lane = row: alu_row fills it in
    X(BIT, "mbcnt_u32_b32", "v_mbcnt_hi_u32_b32", "V1_MBCNT", "INT", lambda s: s[2])
    sat8 = lambda v, n, lo, hi: _sat(_sx(v, 32) >> (n & 31), lo, hi) & 255  # noqa: E731
    X(BIT, "ashr_pk_i8_i32", "v_ashr_pk_i8_i32", "V1_VVVO", "INT", lambda s: (
        (s[3] & 0xFFFF0000) | sat8(s[0], s[2], -128, 127) | (sat8(s[1], s[2], -128, 127) << 8)))
    X(BIT, "ashr_pk_u8_i32", "v_ashr_pk_u8_i32", "V1_VVVO", "INT", lambda s: (
        (s[3] & 0xFFFF0000) | sat8(s[0], s[2], 0, 255) | (sat8(s[1], s[2], 0, 255) << 8)))
    # pk_int
    pk = lambda name, sig, fn: X(PKINT, name, "v_" + name, sig, "INT", _halves(fn))  # noqa: E731
    pk("pk_add_u16", "V1_VV", lambda x, y, z: x + y)
    pk("pk_sub_i16", "V1_VV", lambda x, y, z: x - y)
    pk("pk_mul_lo_u16", "V1_VV", lambda x, y, z: x * y)
    pk("pk_mad_i16", "V1_VVV", lambda x, y, z: _sx(x, 16) * _sx(y, 16) + _sx(z, 16))
    pk("pk_mad_u16", "V1_VVV", lambda x, y, z: x * y + z)
    pk("pk_min_i16", "V1_VV", lambda x, y, z: x if _sx(x, 16) < _sx(y, 16) else y)
    pk("pk_max_i16", "V1_VV", lambda x, y, z: x if _sx(x, 16) > _sx(y, 16) else y)
    pk("pk_min_u16", "V1_VV", lambda x, y, z: min(x, y))
    pk("pk_max_u16", "V1_VV", lambda x, y, z: max(x, y))
    pk("pk_lshlrev_b16", "V1_VV", lambda x, y, z: y << (x & 15))
    pk("pk_ashrrev_i16", "V1_VV", lambda x, y, z: _sx(y, 16) >> (x & 15))
    X(PKINT, "pk_add_u16_opsel", "v_pk_add_u16", "V1_VV", "INT", lambda s: (
        (((s[0] >> 16) + s[1]) & 0xFFFF) | (((s[0] + (s[1] >> 16)) & 0xFFFF) << 16)))
    X(PKINT, "pk_mul_lo_u16_opsel", "v_pk_mul_lo_u16", "V1_VV", "INT", lambda s: (
        (((s[0] & 0xFFFF) * (s[1] >> 16)) & 0xFFFF)
        | ((((s[0] >> 16) * (s[1] & 0xFFFF)) & 0xFFFF) << 16)))
    X(PKINT, "add_u32_sdwa", "v_add_u32_sdwa", "V1_VVO", "INT", lambda s: (
        (s[2] & 0xFFFF) | (((((s[0] >> 16) & 255) + _sx(s[1], 16)) & 0xFFFF) << 16)))
    X(PKINT, "sub_u32_sdwa", "v_sub_u32_sdwa", "V1_VVO", "INT", lambda s: (
        (s[2] & 0xFFFF00FF) | ((((s[0] >> 16) - (s[1] >> 24)) & 255) << 8)))
    # dot
    X(DOT, "dot4_i32_i8", "v_dot4_i32_i8", "V1_VVV", "INT", lambda s: _dot(s, 4, 8, True))
    X(DOT, "dot4_u32_u8", "v_dot4_u32_u8", "V1_VVV", "INT", lambda s: _dot(s, 4, 8, False))
    X(DOT, "dot8_i32_i4", "v_dot8_i32_i4", "V1_VVV", "INT", lambda s: _dot(s, 8, 4, True))
    X(DOT, "dot8_u32_u4", "v_dot8_u32_u4", "V1_VVV", "INT", lambda s: _dot(s, 8, 4, False))
    X(DOT, "dot2_i32_i16", "v_dot2_i32_i16", "V1_VVV", "INT", lambda s: _dot(s, 2, 16, True))
    X(DOT, "dot2_u32_u16", "v_dot2_u32_u16", "V1_VVV", "INT", lambda s: _dot(s, 2, 16, False))
    X(DOT, "dot2_f32_f16", "v_dot2_f32_f16", "V1_VVV", "DOTF16", lambda s: u32_of(
        half(s[0]) * half(s[1]) + half(s[0] >> 16) * half(s[1] >> 16) + f32(s[2])))
    bdot = lambda s: u32_of(  # noqa: E731
        bf16(s[0]) * bf16(s[1]) + bf16(s[0] >> 16) * bf16(s[1] >> 16) + f32(s[2]))
    X(DOT, "dot2_f32_bf16", "v_dot2_f32_bf16", "V1_VVV", "DOTBF16", bdot)
    # f32
    fma = lambda a, b, c: u32_of(f32(a) * f32(b) + f32(c))  # noqa: E731  exact in f64
    X(F32, "add_f32", "v_add_f32", "V1_VV", "F32", lambda s: add(s[0], s[1]))
    X(F32, "sub_f32", "v_sub_f32", "V1_VV", "F32", lambda s: sub(s[0], s[1]))
    X(F32, "mul_f32", "v_mul_f32", "V1_VV", "F32", lambda s: mul(s[0], s[1]))
    X(F32, "fma_f32", "v_fma_f32", "V1_VVV", "F32FMA", lambda s: fma(s[0], s[1], s[2]))
    X(F32, "pk_fma_f32", "v_pk_fma_f32", "V2_DDD", "F32PKFMA",
      lambda s: (fma(s[0], s[2], s[4]), fma(s[1], s[3], s[5])))
    X(F32, "pk_mul_f32", "v_pk_mul_f32", "V2_DD", "F32",
      lambda s: (mul(s[0], s[2]), mul(s[1], s[3])))
    X(F32, "pk_add_f32", "v_pk_add_f32", "V2_DD", "F32",
      lambda s: (add(s[0], s[2]), add(s[1], s[3])))
    X(F32, "add_f32_negabs", "v_add_f32", "V1_VV", "F32",
      lambda s: add(s[0] ^ 0x80000000, s[1] & 0x7FFFFFFF))
    X(F32, "mul_f32_clamp", "v_mul_f32", "V1_VV", "F32", _clamp01)
    X(F32, "fma_f32_neg", "v_fma_f32", "V1_VVV", "F32FMA",
      lambda s: fma(s[0], s[1] ^ 0x80000000, s[2] & 0x7FFFFFFF))
    f3 = lambda s: (f32(s[0]), f32(s[1]), f32(s[2]))  # noqa: E731
    X(F32, "min_f32", "v_min_f32", "V1_VV", "F32", lambda s: u32_of(_fmin(f32(s[0]), f32(s[1]))))
    X(F32, "max_f32", "v_max_f32", "V1_VV", "F32", lambda s: u32_of(_fmax(f32(s[0]), f32(s[1]))))
    X(F32, "med3_f32", "v_med3_f32", "V1_VVV", "F32", lambda s: u32_of(
        _fmax(_fmin(*f3(s)[:2]), _fmin(_fmax(*f3(s)[:2]), f3(s)[2]))))
    X(F32, "minimum3_f32", "v_minimum3_f32", "V1_VVV", "F32",
      lambda s: u32_of(_fmin(_fmin(*f3(s)[:2]), f3(s)[2])))
    X(F32, "maximum3_f32", "v_maximum3_f32", "V1_VVV", "F32",
      lambda s: u32_of(_fmax(_fmax(*f3(s)[:2]), f3(s)[2])))
    X(F32, "ldexp_f32", "v_ldexp_f32", "V1_VV", "F32I",
      lambda s: u32_of(_ldexp(f32(s[0]), _sx(s[1], 32))))
    X(F32, "frexp_mant_f32", "v_frexp_mant_f32", "V1_V", "F32",
      lambda s: u32_of(math.frexp(f32(s[0]))[0]))
    X(F32, "frexp_exp_i32_f32", "v_frexp_exp_i32_f32", "V1_V", "F32", _frexp_exp)
    X(F32, "fract_f32", "v_fract_f32", "V1_V", "F32", _fract)
    for name, fn in (("floor", np.floor), ("ceil", np.ceil), ("trunc", np.trunc),
                     ("rndne", np.rint)):
        X(F32, f"{name}_f32", f"v_{name}_f32", "V1_V", "F32", lambda s, op=_f32op(fn): op(s[0]))
    # f16
    X(F16, "pk_fma_f16", "v_pk_fma_f16", "V1_VVV", "F16FMA", _fhalves(lambda x, y, z: x * y + z))
    X(F16, "pk_add_f16", "v_pk_add_f16", "V1_VV", "F16", _fhalves(lambda x, y, z: x + y))
    X(F16, "pk_mul_f16", "v_pk_mul_f16", "V1_VV", "F16", _fhalves(lambda x, y, z: x * y))
    X(F16, "pk_min_f16", "v_pk_min_f16", "V1_VV", "F16", _fhalves(lambda x, y, z: _fmin(x, y)))
    X(F16, "pk_max_f16", "v_pk_max_f16", "V1_VV", "F16", _fhalves(lambda x, y, z: _fmax(x, y)))
    # v_fma_f16 keeps the destination's high half: `old` is a payload
    X(F16, "fma_f16", "v_fma_f16", "V1_VVVO", "F16FMA",
      lambda s: (s[3] & 0xFFFF0000) | half_of(half(s[0]) * half(s[1]) + half(s[2])))
    X(F16, "fma_mix_f32", "v_fma_mix_f32", "V1_VVV", "F16FMA",
      lambda s: u32_of(half(s[0]) * half(s[1] >> 16) + half(s[2])))
    X(F16, "fma_mixlo_f16", "v_fma_mixlo_f16", "V1_VVVO", "F16FMA", lambda s: (
        (s[3] & 0xFFFF0000) | half_of(half(s[0] >> 16) * half(s[1]) + half(s[2] >> 16))))
    X(F16, "fma_mixhi_f16", "v_fma_mixhi_f16", "V1_VVVO", "F16FMA", lambda s: (
        (s[3] & 0xFFFF) | (half_of(half(s[0]) * half(s[1] >> 16) + half(s[2] >> 16)) << 16)))
    # f64 (Python floats are IEEE doubles)
    da, db, dc = (lambda s: f64(s[0], s[1])), (lambda s: f64(s[2], s[3])), (lambda s: f64(s[4], s[5]))
    X(F64, "add_f64", "v_add_f64", "V2_DD", "F64", lambda s: _wd(da(s) + db(s)))
    X(F64, "mul_f64", "v_mul_f64", "V2_DD", "F64", lambda s: _wd(da(s) * db(s)))
    X(F64, "fma_f64", "v_fma_f64", "V2_DDD", "F64FMA", lambda s: _wd(da(s) * db(s) + dc(s)))
    X(F64, "min_f64", "v_min_f64", "V2_DD", "F64", lambda s: _wd(_fmin(da(s), db(s))))
    X(F64, "max_f64", "v_max_f64", "V2_DD", "F64", lambda s: _wd(_fmax(da(s), db(s))))
    X(F64, "ldexp_f64", "v_ldexp_f64", "V2_DV", "F64I",
      lambda s: _wd(_ldexp(da(s), _sx(s[2], 32))))
    X(F64, "frexp_mant_f64", "v_frexp_mant_f64", "V2_D", "F64R",
      lambda s: _wd(math.frexp(da(s))[0]))
    X(F64, "trunc_f64", "v_trunc_f64", "V2_D", "F64R", lambda s: _wd(float(np.trunc(da(s)))))
    X(F64, "floor_f64", "v_floor_f64", "V2_D", "F64R", lambda s: _wd(float(np.floor(da(s)))))
    X(F64, "rndne_f64", "v_rndne_f64", "V2_D", "F64R", lambda s: _wd(float(np.rint(da(s)))))
    X(F64, "div_f64", "v_div_fixup_f64", "X_DIV", "F64DIV", _div_f64)
    X(F64, "sqrt_f64", "v_rsq_f64", "X_SQRT", "F64DIV", lambda s: _wd(math.sqrt(da(s))))
    # convert
    X(CVT, "cvt_f32_i32", "v_cvt_f32_i32", "V1_V", "INT", lambda s: u32_of(float(_sx(s[0], 32))))
    X(CVT, "cvt_f32_u32", "v_cvt_f32_u32", "V1_V", "INT", lambda s: u32_of(float(s[0])))
    X(CVT, "cvt_i32_f32", "v_cvt_i32_f32", "V1_V", "F32CVT",
      lambda s: _cvt_int(f32(s[0]), -2 ** 31, 2 ** 31 - 1))
    X(CVT, "cvt_u32_f32", "v_cvt_u32_f32", "V1_V", "F32CVT",
      lambda s: _cvt_int(f32(s[0]), 0, 2 ** 32 - 1))
    X(CVT, "cvt_f16_f32", "v_cvt_f16_f32", "V1_V", "F32H", lambda s: half_of(f32(s[0])))
    X(CVT, "cvt_f32_f16", "v_cvt_f32_f16", "V1_V", "F16", lambda s: u32_of(half(s[0])))
    X(CVT, "cvt_pkrtz_f16_f32", "v_cvt_pkrtz_f16_f32", "V1_VV", "F32H",
      lambda s: half_of(f32(s[0]), True) | (half_of(f32(s[1]), True) << 16))
    X(CVT, "cvt_pk_bf16_f32", "v_cvt_pk_bf16_f32", "V1_VV", "F32",
      lambda s: bf16_of(s[0]) | (bf16_of(s[1]) << 16))
    X(CVT, "cvt_f64_f32", "v_cvt_f64_f32", "V2_V", "F32", lambda s: _wd(f32(s[0])))
    X(CVT, "cvt_f32_f64", "v_cvt_f32_f64", "V1_D", "F64R", lambda s: u32_of(da(s)))
    X(CVT, "cvt_f64_i32", "v_cvt_f64_i32", "V2_V", "INT", lambda s: _wd(float(_sx(s[0], 32))))
    X(CVT, "cvt_i32_f64", "v_cvt_i32_f64", "V1_D", "F64R",
      lambda s: _cvt_int(da(s), -2 ** 31, 2 ** 31 - 1))
    for i in range(4):
        X(CVT, f"cvt_f32_ubyte{i}", f"v_cvt_f32_ubyte{i}", "V1_V", "INT",
          lambda s, i=i: u32_of(float((s[0] >> (8 * i)) & 255)))
    X(CVT, "cvt_pk_i16_i32", "v_cvt_pk_i16_i32", "V1_VV", "INT", lambda s: (
        (_sat(_sx(s[0], 32), -32768, 32767) & 0xFFFF)
        | ((_sat(_sx(s[1], 32), -32768, 32767) & 0xFFFF) << 16)))
    X(CVT, "cvt_pk_u16_u32", "v_cvt_pk_u16_u32", "V1_VV", "INT",
      lambda s: min(s[0], 0xFFFF) | (min(s[1], 0xFFFF) << 16))
    X(CVT, "cvt_pk_u8_f32", "v_cvt_pk_u8_f32", "V1_VVV", "F32U8", _cvt_pk_u8)
    snorm = lambda b: int(np.rint(min(max(f32(b), -1.0), 1.0) * 32767.0)) & 0xFFFF  # noqa: E731
    X(CVT, "cvt_pknorm_i16_f32", "v_cvt_pknorm_i16_f32", "V1_VV", "F32NORM",
      lambda s: snorm(s[0]) | (snorm(s[1]) << 16))
    # scale_convert
    E4M3, E5M2, E2M1 = 0, 1, 4
    X(SCALE, "sc_pk_f32_fp8", "v_cvt_scalef32_pk_f32_fp8", "V2_VV", "FP8",
      lambda s: (_dec(E4M3, s[0] & 255, s[1]), _dec(E4M3, (s[0] >> 8) & 255, s[1])))
    X(SCALE, "sc_pk32_f32_fp6_x2", "v_cvt_scalef32_pk32_f32_fp6", "V2_FP6", "FP6",
      lambda s: _fp6_fold(s, 0x40000000))
    X(SCALE, "sc_pk32_f32_fp6_half", "v_cvt_scalef32_pk32_f32_fp6", "V2_FP6", "FP6",
      lambda s: _fp6_fold(s, 0x3F000000))
    X(SCALE, "sc_pk_fp8_f16", "v_cvt_scalef32_pk_fp8_f16", "V1_VVO", "SCALEF16", lambda s: (
        (s[2] & 0xFFFF0000) | _encd(0, half(s[0]), s[1], 0x7F)
        | (_encd(0, half(s[0] >> 16), s[1], 0x7F) << 8)))
    X(SCALE, "sc_pk_fp8_bf16", "v_cvt_scalef32_pk_fp8_bf16", "V1_VVO", "SCALEBF16", lambda s: (
        (s[2] & 0xFFFF0000) | _encd(0, bf16(s[0]), s[1], 0x7F)
        | (_encd(0, bf16(s[0] >> 16), s[1], 0x7F) << 8)))
    X(SCALE, "sc_pk_f32_fp8_hi", "v_cvt_scalef32_pk_f32_fp8", "V2_VV", "FP8",
      lambda s: (_dec(E4M3, (s[0] >> 16) & 255, s[1]), _dec(E4M3, s[0] >> 24, s[1])))
    X(SCALE, "sc_pk_f32_bf8", "v_cvt_scalef32_pk_f32_bf8", "V2_VV", "BF8",
      lambda s: (_dec(E5M2, s[0] & 255, s[1]), _dec(E5M2, (s[0] >> 8) & 255, s[1])))
    X(SCALE, "sc_pk_f32_fp4", "v_cvt_scalef32_pk_f32_fp4", "V2_VV", "FP4",
      lambda s: (_dec(E2M1, s[0] & 15, s[1]), _dec(E2M1, (s[0] >> 4) & 15, s[1])))
    enc2 = lambda s, fmt, mx, sh: (  # noqa: E731
        _enc(fmt, s[0], s[2], mx) | (_enc(fmt, s[1], s[2], mx) << sh))
    X(SCALE, "sc_pk_fp8_f32", "v_cvt_scalef32_pk_fp8_f32", "V1_VVVO", "SCALEF32",
      lambda s: (s[3] & 0xFFFF0000) | enc2(s, E4M3, 0x7F, 8))
    X(SCALE, "sc_pk_fp8_f32_hi", "v_cvt_scalef32_pk_fp8_f32", "V1_VVVO", "SCALEF32",
      lambda s: (s[3] & 0xFFFF) | (enc2(s, E4M3, 0x7F, 8) << 16))
    X(SCALE, "sc_pk_bf8_f32", "v_cvt_scalef32_pk_bf8_f32", "V1_VVVO", "SCALEF32",
      lambda s: (s[3] & 0xFFFF0000) | enc2(s, E5M2, 0x7C, 8))
    X(SCALE, "sc_pk_fp4_f32", "v_cvt_scalef32_pk_fp4_f32", "V1_VVVO", "SCALEF32",
      lambda s: (s[3] & 0xFFFFFF00) | enc2(s, E2M1, 7, 4))
    # compare_select
    cmp = lambda p, rel: int(rel & _PRED[p] != 0)  # noqa: E731
    for p in ("lt", "le", "eq", "lg", "gt", "ge", "o", "u", "nge", "nlt"):
        X(CMP, f"cmp_{p}_f32", f"v_cmp_{p}_f32", "V1_VV", "CMPF32",
          lambda s, p=p: cmp(p, _rel(f32(s[0]), f32(s[1]))))
    for p in ("lt", "le", "eq", "lg", "gt", "ge"):
        X(CMP, f"cmp_{p}_f64", f"v_cmp_{p}_f64", "V1_DD", "CMPF64",
          lambda s, p=p: cmp(p, _rel(da(s), db(s))))
    for p in ("lt", "le", "eq", "lg", "gt", "ge"):
        X(CMP, f"cmp_{p}_f16", f"v_cmp_{p}_f16", "V1_VV", "CMPF16",
          lambda s, p=p: cmp(p, _rel(half(s[0]), half(s[1]))))
    for p in ("lt", "eq", "gt", "ne"):
        X(CMP, f"cmp_{p}_i32", f"v_cmp_{p}_i32", "V1_VV", "CMPINT",
          lambda s, p=p: cmp(p, _rel(_sx(s[0], 32), _sx(s[1], 32))))
        X(CMP, f"cmp_{p}_u32", f"v_cmp_{p}_u32", "V1_VV", "CMPINT",
          lambda s, p=p: cmp(p, _rel(s[0], s[1])))
        X(CMP, f"cmp_{p}_i64", f"v_cmp_{p}_i64", "V1_DD", "CMPINT",
          lambda s, p=p: cmp(p, _rel(_sx(_A(s), 64), _sx(_B(s), 64))))
        X(CMP, f"cmp_{p}_u64", f"v_cmp_{p}_u64", "V1_DD", "CMPINT",
          lambda s, p=p: cmp(p, _rel(_A(s), _B(s))))
    X(CMP, "cmp_class_f32", "v_cmp_class_f32", "V1_VV", "CLASS32",
      lambda s: (s[1] >> _class(s[0], 8, 23)) & 1)
    X(CMP, "cmp_class_f64", "v_cmp_class_f64", "V1_DV", "CLASS64",
      lambda s: (s[2] >> _class(_A(s), 11, 52)) & 1)
    X(CMP, "cmpx_lt_u32", "v_cmpx_lt_u32", "V1_CMPX", "INT",
      lambda s: s[0] if s[0] < s[1] else s[2])
    # salu
    S = lambda name, sig, ref, cls="INT", mnem=None: X(  # noqa: E731
        SALU, name, mnem or name, sig, cls, ref)
    S("s_add_u64", "S2C_SSSS", lambda s: _w64((((s[2] << 32) | s[0]) + ((s[3] << 32) | s[1])) & M64),
      mnem="s_addc_u32")
    S("s_sub_u64", "S2C_SSSS", lambda s: _w64((((s[2] << 32) | s[0]) - ((s[3] << 32) | s[1])) & M64),
      mnem="s_subb_u32")
    S("s_mul_i32", "S1_SS", lambda s: (s[0] * s[1]) & M32)
    S("s_mul_hi_u32", "S1_SS", lambda s: (s[0] * s[1]) >> 32)
    S("s_mul_hi_i32", "S1_SS", lambda s: ((_sx(s[0], 32) * _sx(s[1], 32)) >> 32) & M32)
    S("s_lshl_b32", "S1C_SS", _scc(lambda s: s[0] << (s[1] & 31)))
    S("s_lshr_b32", "S1C_SS", _scc(lambda s: s[0] >> (s[1] & 31)))
    S("s_ashr_i32", "S1C_SS", _scc(lambda s: _sx(s[0], 32) >> (s[1] & 31)))
    S("s_lshl_b64", "S2_QS", lambda s: _w64((_A(s) << (s[2] & 63)) & M64))
    S("s_lshr_b64", "S2_QS", lambda s: _w64(_A(s) >> (s[2] & 63)))
    S("s_ashr_i64", "S2_QS", lambda s: _w64((_sx(_A(s), 64) >> (s[2] & 63)) & M64))
    logic = (("and", lambda a, b: a & b), ("or", lambda a, b: a | b), ("xor", lambda a, b: a ^ b),
             ("nand", lambda a, b: ~(a & b)), ("nor", lambda a, b: ~(a | b)),
             ("xnor", lambda a, b: ~(a ^ b)), ("andn2", lambda a, b: a & ~b),
             ("orn2", lambda a, b: a | ~b))
    for name, fn in logic:
        S(f"s_{name}_b32", "S1C_SS", _scc(lambda s, fn=fn: fn(s[0], s[1])))
    for name, fn in logic:
        S(f"s_{name}_b64", "S2_QQ", lambda s, fn=fn: _w64(fn(_A(s), _B(s)) & M64))
    S("s_not_b32", "S1C_S", _scc(lambda s: ~s[0]))
    S("s_brev_b32", "S1_S", lambda s: _rev(s[0]))
    S("s_brev_b64", "S2_Q", lambda s: (_rev(s[1]), _rev(s[0])))
    S("s_bcnt0_i32_b32", "S1C_S", _scc(lambda s: 32 - _pop(s[0])))
    S("s_bcnt1_i32_b64", "S1C_Q", _scc(lambda s: _pop(_A(s))))
    S("s_ff0_i32_b32", "S1_S", lambda s: _ctz(s[0] ^ M32) if s[0] != M32 else M32)
    S("s_ff1_i32_b32", "S1_S", lambda s: _ctz(s[0]) if s[0] else M32)
    S("s_ff1_i32_b64", "S1_Q", lambda s: _ctz(_A(s)) if _A(s) else M32)
    S("s_flbit_i32_b32", "S1_S", lambda s: _clz(s[0]) if s[0] else M32)
    S("s_flbit_i32", "S1_S", lambda s: _flbit_i32(s[0]))
    S("s_flbit_i32_b64", "S1_Q", lambda s: 64 - _A(s).bit_length() if _A(s) else M32)
    S("s_sext_i32_i8", "S1_S", lambda s: _sx(s[0], 8) & M32)
    S("s_sext_i32_i16", "S1_S", lambda s: _sx(s[0], 16) & M32)
    S("s_bfm_b32", "S1_SS", lambda s: (((1 << (s[0] & 31)) - 1) << (s[1] & 31)) & M32)
    S("s_bfe_u32", "S1C_SS", _s_bfe_u32)
    S("s_bfe_i32", "S1C_SS", _s_bfe_i32)
    S("s_bfe_u64", "S2_QS", lambda s: _w64(_bfe64(_A(s), s[2], False)))
    S("s_bfe_i64", "S2_QS", lambda s: _w64(_bfe64(_A(s), s[2], True)))
    # SCC of the forms whose result fills both words
    for name, fn in logic:
        S(f"s_{name}_b64_scc", "SC_QQ", lambda s, fn=fn: int(fn(_A(s), _B(s)) & M64 != 0),
          mnem=f"s_{name}_b64")
    S("s_lshl_b64_scc", "SC_QS", lambda s: int((_A(s) << (s[2] & 63)) & M64 != 0), mnem="s_lshl_b64")
    S("s_lshr_b64_scc", "SC_QS", lambda s: int(_A(s) >> (s[2] & 63) != 0), mnem="s_lshr_b64")
    S("s_ashr_i64_scc", "SC_QS", lambda s: int(_sx(_A(s), 64) >> (s[2] & 63) != 0),
      mnem="s_ashr_i64")
    S("s_bfe_u64_scc", "SC_QS", lambda s: int(_bfe64(_A(s), s[2], False) != 0), mnem="s_bfe_u64")
    S("s_bfe_i64_scc", "SC_QS", lambda s: int(_bfe64(_A(s), s[2], True) != 0), mnem="s_bfe_i64")
    S("s_add_u64_scc", "SC_SSSS", lambda s: int(
        ((s[2] << 32) | s[0]) + ((s[3] << 32) | s[1]) > M64), mnem="s_addc_u32")
    S("s_sub_u64_scc", "SC_SSSS", lambda s: int(
        ((s[2] << 32) | s[0]) < ((s[3] << 32) | s[1])), mnem="s_subb_u32")
    for t, sign in (("i32", True), ("u32", False)):
        for p in ("eq", "lg", "lt", "gt"):
            S(f"s_cselect_{p}_{t}", "S1_SSSS", lambda s, p=p, sign=sign: (
                s[2] if cmp(p, _rel(*((_sx(s[0], 32), _sx(s[1], 32)) if sign else (s[0], s[1]))))
                else s[3]), cls="CMPINT", mnem=f"s_cmp_{p}_{t}")
    S("s_absdiff_i32", "S1C_SS", _scc(lambda s: abs(_sx(s[0] - s[1], 32))))
    S("s_min_i32", "S1C_SS", lambda s: (
        (s[0], 1) if _sx(s[0], 32) < _sx(s[1], 32) else (s[1], 0)))
    S("s_max_u32", "S1C_SS", lambda s: (s[0], 1) if s[0] > s[1] else (s[1], 0))
    for n in (1, 2, 3, 4):
        S(f"s_lshl{n}_add_u32", "S1C_SS", _lshl_add(n))
    S("s_pack_ll_b32_b16", "S1_SS", lambda s: (s[0] & 0xFFFF) | ((s[1] << 16) & M32))
    S("s_pack_lh_b32_b16", "S1_SS", lambda s: (s[0] & 0xFFFF) | (s[1] & 0xFFFF0000))
    S("s_pack_hh_b32_b16", "S1_SS", lambda s: (s[0] >> 16) | (s[1] & 0xFFFF0000))
    # transcendental
    T = lambda op, sig, cls, ref: X(TRANS, "t_" + op, "v_" + op, sig, cls, ref)  # noqa: E731
    t32 = lambda fn: (lambda s: u32_of(_exact_t(fn)(f32(s[0]))))  # noqa: E731
    t64 = lambda fn: (lambda s: _wd(_exact_t(fn)(da(s))))  # noqa: E731
    t16 = lambda fn: (lambda s: half_of(_exact_t(fn)(half(s[0]))))  # noqa: E731
    T("exp_f32", "V1_V", "TEXP", t32(lambda x: 2.0 ** x))
    T("log_f32", "V1_V", "TLOG", t32(math.log2))
    T("rcp_f32", "V1_V", "TRCP", t32(lambda x: 1.0 / x))
    T("rsq_f32", "V1_V", "TSQRT", t32(lambda x: 1.0 / math.sqrt(x)))
    T("sqrt_f32", "V1_V", "TSQRT", t32(math.sqrt))
    T("sin_f32", "V1_V", "TSIN", t32(_sinrev))
    T("cos_f32", "V1_V", "TSIN", t32(_cosrev))
    T("rcp_f64", "V2_D", "TRCP64", t64(lambda x: 1.0 / x))
    T("rsq_f64", "V2_D", "TSQRT64", t64(lambda x: 1.0 / math.sqrt(x)))
    T("sqrt_f64", "V2_D", "TSQRT64", t64(math.sqrt))
    T("exp_f16", "V1_V", "TEXP16", t16(lambda x: 2.0 ** x))
    T("log_f16", "V1_V", "TLOG16", t16(math.log2))
    T("rcp_f16", "V1_V", "TRCP16", t16(lambda x: 1.0 / x))
    T("sqrt_f16", "V1_V", "TSQRT16", t16(math.sqrt))
    return F


_forms = None


def alu_forms():
    """The form list: (check, name, mnemonic, signature, class, reference)."""
    global _forms
    if _forms is None:
        _forms = _build_forms()
    return _forms


def form_index(name: str) -> int:
    return [f[1] for f in alu_forms()].index(name)


def is_scalar(form: int) -> bool:
    return alu_forms()[form][3].startswith("S")


def checked_rows(form: int) -> int:
    """Rows whose result words are compared: all, of a transcendental form
    its anchors; v_sqrt_f64 (not exact on its anchors) has none."""
    check, name = alu_forms()[form][:2]
    if check != TRANS:
        return ROWS
    return 0 if name == "t_sqrt_f64" else ANCHORS


def alu_elem(form: int, word: int, row: int, lane: int) -> int:
    return (form << 13) | (word << 12) | (row << 6) | lane


def decode_first_bad(first_bad: int) -> dict:
    return {"form": first_bad >> 13, "word": (first_bad >> 12) & 1,
            "row": (first_bad >> 6) & 63, "lane": first_bad & 63}


# -- operand rows ----------------------------------------------------------------------

INT_EDGES = (
    (0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 1, 1), (M32,) * 6,
    (0x80000000, 0x80000000, 0x80000000, 0x80000000, 1, 0),
    (0x0000FFFF, 1, 0x0000FFFF, 0, 1, 0), (0x00FFFFFF, 1, 0x00FFFFFF, 0, 1, 0),
    (0xFFFFFFFF, 1, 0xFFFFFFFF, 0, 1, 0),
    (0, 0x12345678, 0x9ABCDEF0, 0, 0x0F0F0F0F, 0), (31, 0x12345678, 0x9ABCDEF0, 31, 0x0F0F0F0F, 31),
    (32, 0x12345678, 0x9ABCDEF0, 32, 0x0F0F0F0F, 32), (63, 0x12345678, 0x9ABCDEF0, 63, 0x0F0F0F0F, 63),
    (0x92345678, 0, 0, 0x9ABCDEF0, 0, 0), (0x92345678, 31, 31, 0x9ABCDEF0, 31, 31),
    (0x92345678, 32, 32, 0x9ABCDEF0, 32, 32), (0x92345678, 63, 63, 0x9ABCDEF0, 63, 63),
)
F32_EDGES = (
    (0x00000000, 0x80000000, 0x00000000), (0x80000000, 0x80000000, 0x00000000),
    (0x00800000, 0x00800000, 0x80800000), (0x7F7FFFFF, 0x7F7FFFFF, 0x7F7FFFFF),
    (0x00000001, 0x00000001, 0x80000001), (0x007FFFFF, 0x00000001, 0x807FFFFF),
    (0x3F800000, 0x33800000, 0x00000000), (0x3F800001, 0x33800000, 0x80000000),
    (0x7F7FFFFF, 0x73000000, 0x3F800000), (0xFF7FFFFF, 0xFF7FFFFF, 0x3F800000),
    (0x3F801000, 0x3F801000, 0x3F800000), (0x00800000, 0x3F000000, 0x00000001),
    (0xBFC00000, 0x40200000, 0x3F000000), (0x807FFFFF, 0x00800000, 0x3FC00000),
)
FMA_EDGES = (
    (0x3F800000, 0x3F800000, 0x33800000), (0x3F800001, 0x3F800000, 0x33800000),
    (0x00000000, 0x80000000, 0x00000000), (0x00800000, 0x3F800000, 0x00000001),
    (0x007FFFFF, 0x3F800000, 0x80000001), (0x7F7FFFFF, 0x3F800000, 0x73000000),
    (0x3F801000, 0x3F801000, 0xB3800000), (0x1E000000, 0x1E000000, 0x00000003),
)
F32I_EDGES = ((0x00000001, 10), (0x7F7FFFFF, 1), (0x3F800000, -149 & M32), (0x3F800000, -150 & M32),
              (0x40400000, -150 & M32), (0x80000000, 5))
F32CVT_EDGES = (0x7FC00000, 0x7F800000, 0xFF800000, 0x4F000000, 0xCF000000, 0x4F800000,
                0x4EFFFFFF, 0xBF800000, 0x3F7FFFFF, 0x00000000, 0x80000000, 0xCF000001)
F32H_EDGES = (0x3F801000, 0x3F803000, 0x477FF000, 0x477FEFFF, 0x33000000, 0x33800000, 0x33C00000,
              0x38800000, 0x80000000, 0x387FC000)
F16_EDGES = ((0x80000000, 0x00008000), (0x04000400, 0x04000400), (0x7BFF7BFF, 0x7BFF7BFF),
             (0x00010001, 0x00018001), (0x03FF03FF, 0x00018001), (0x3C003C01, 0x10001000),
             (0x7BFF7BFF, 0x5000D000), (0x3C013C01, 0x3C013C01))
F64_EDGES = (
    (0x0000000000000000, 0x8000000000000000), (0x0010000000000000, 0x0010000000000000),
    (0x7FEFFFFFFFFFFFFF, 0x7FEFFFFFFFFFFFFF), (0x0000000000000001, 0x0000000000000001),
    (0x000FFFFFFFFFFFFF, 0x8000000000000001), (0x3FF0000000000000, 0x3CA0000000000000),
    (0x3FF0000000000001, 0x3CA0000000000000), (0x7FEFFFFFFFFFFFFF, 0x7C90000000000000),
    (0x3FF8000000000000, 0x0000000000000003), (0x7E37E43C8800759C, 0x3EB0000000000000),
)
F32U8_EDGES = (0x3F000000, 0x3FC00000, 0x40200000, 0x437F8000, 0x43800000, 0xBF800000, 0x437E8000,
               0x80000000, 0x00000001, 0x437F0000)
F32NORM_EDGES = (0x3F800000, 0xBF800000, 0x40000000, 0xC0000000, 0x00000000, 0x80000000, 0x3F000000,
                 0x37800100)
SCALE16_EDGES = ((30000, -30000), (464, 480), (0, 0), (17, 19))
F16FMA_EDGES = ((0x3C003C00, 0x3C013C00, 0x10001000), (0x00008000, 0x3C003C00, 0x80000000),
                (0x00010001, 0x3C003C00, 0x800103FF), (0x04003800, 0x38000001, 0x00010001),
                (0x7BFF7BFF, 0x3C003C00, 0x4C004BFF), (0x7BFFFBFF, 0x3C00BC00, 0x00000000))
F64FMA_EDGES = (
    (0x0000000000000000, 0x8000000000000000, 0x0000000000000000),
    (0x0000000000000001, 0x3FF0000000000000, 0x8000000000000003),
    (0x0010000000000000, 0x3FF0000000000000, 0x0000000000000001),
    (0x7FEFFFFFFFFFFFFF, 0x3FF0000000000000, 0x0000000000000000),
    (0x3FF0000000000000, 0x3FF0000000000000, 0x3CA0000000000000),
    (0x3FF0000000000001, 0x3FF0000000000000, 0x3CA0000000000000),
    (0x7FE0000000000000, 0x4000000000000000, 0x7FE0000000000000),
)
SCALEF32_EDGES = ((0x47000000, 0xC7000000), (0x43E00000, 0x43F00000), (0x3F880000, 0x3F980000),
                  (0x00000000, 0x80000000), (0x3FA00000, 0x40200000), (0x3A800000, 0x3B400000))
CMP_F32 = (0x7FC00000, 0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x3F800001, 0x7F800000,
           0xFF800000, 0x00000001, 0x80000001, 0x7F800001, 0x42280000)
CMP_F16 = (0x0000, 0x8000, 0x3C00, 0xBC00, 0x3C01, 0x0001, 0x8001, 0x7BFF)
CMP_F64 = (0x0000000000000000, 0x8000000000000000, 0x3FF0000000000000, 0xBFF0000000000000,
           0x3FF0000000000001, 0x0000000000000001, 0x8000000000000001, 0x7FEFFFFFFFFFFFFF)
CLASS_F32 = (0x7F800001, 0x7FC00000, 0xFF800000, 0xC0490FDB, 0x80000400, 0x80000000, 0x00000000,
             0x00000400, 0x40490FDB, 0x7F800000)
CLASS_F64 = (0x7FF0000000000001, 0x7FF8000000000000, 0xFFF0000000000000, 0xC00921FB54442D18,
             0x8000000000000400, 0x8000000000000000, 0x0000000000000000, 0x0000000000000400,
             0x400921FB54442D18, 0x7FF0000000000000)


def _f32_bits(x, e_lo, e_n):
    return (x & 0x80000000) | ((127 + e_lo + ((x >> 23) & 255) % e_n) << 23) | (x & 0x7FFFFF)


def _f16_bits(x, e_lo, e_n):
    return (x & 0x8000) | ((15 + e_lo + ((x >> 10) & 31) % e_n) << 10) | (x & 0x3FF)


def _fma_triple(x, y, z):
    a, b = _f32_bits(x, -8, 17), _f32_bits(y, -8, 17)
    eab = ((a >> 23) & 255) + ((b >> 23) & 255) - 254
    return a, b, (z & 0x807FFFFF) | ((127 + eab + ((z >> 23) & 255) % 9 - 4) << 23)


def _f16_fma_c(a, b, z):
    ec = ((a >> 10) & 31) + ((b >> 10) & 31) - 30 + ((z >> 10) & 31) % 9 - 4
    return (z & 0x83FF) | ((_sat(ec, -14, 15) + 15) << 10)


def _f64_small(x, e_lo, e_n):
    v = math.ldexp(float((x & 0x1FFFFF) | 0x100001), e_lo + ((x >> 21) & 255) % e_n - 20)
    return u64_of(-v if x >> 31 else v)


def _f64_full(x, y, e_lo, e_n):
    return (((x & 0x80000000) << 32) | ((1023 + e_lo + ((x >> 20) & 2047) % e_n) << 52)
            | ((x & 0xFFFFF) << 32) | y)


def alu_sources(seed: int, form: int, row: int) -> list:
    """cro_alu_sources: the six source words of a row."""
    cls = alu_forms()[form][4]
    x = [alu_rand(seed, form, row, k) for k in range(6)]
    scale = u32_of(math.ldexp(1.0, x[5] % 9 - 4))
    s = list(x)
    if cls == "INT":
        if row < len(INT_EDGES):
            s = list(INT_EDGES[row])
    elif cls == "PERM":
        s[2] = 0x03020100 + 0x04040404 * row if row < 4 else x[2] & 0x0F0F0F0F
    elif cls == "F32":
        s = [F32_EDGES[row][k % 3] if row < len(F32_EDGES) else _f32_bits(x[k], -7, 34)
             for k in range(6)]
    elif cls in ("F32FMA", "F32PKFMA"):
        t = []
        for p in range(2):
            t += (FMA_EDGES[(row + p) % 8] if row < 8
                  else _fma_triple(x[3 * p], x[3 * p + 1], x[3 * p + 2]))
        s = t if cls == "F32FMA" else [t[3 * (k & 1) + (k >> 1)] for k in range(6)]
    elif cls == "F32I":
        s[0] = F32I_EDGES[row][0] if row < 6 else _f32_bits(x[0], -20, 41)
        s[1] = F32I_EDGES[row][1] if row < 6 else (x[1] % 81 - 40) & M32
    elif cls == "F32U8":
        s[0] = F32U8_EDGES[row] if row < 10 else _f32_bits(x[0], -3, 12)
        s[1] = row if row < 10 else x[1]
    elif cls == "F32NORM":
        s = [F32NORM_EDGES[(row + k) % 8] if row < 8 else _f32_bits(x[k], -18, 19)
             for k in range(6)]
    elif cls in ("SCALEF16", "SCALEBF16"):
        s[0] = 0
        for h in range(2):
            if row < 4:
                v = SCALE16_EDGES[row][h] / (16.0 if row == 3 else 1.0)
            else:
                v = f32(_f32_bits(x[h], -9, 19) & 0xFFFF0000)
            bits = half_of(v) if cls == "SCALEF16" else u32_of(v) >> 16
            s[0] |= bits << (16 * h)
        if row == 2:
            s[0] = 0x80000000
        s[1] = 0x3F800000 if row < 4 else scale
    elif cls == "F32CVT":
        s = [F32CVT_EDGES[(row + k) % 12] if row < 12 else _f32_bits(x[k], -2, 36)
             for k in range(6)]
    elif cls == "F32H":
        s = [F32H_EDGES[(row + k) % 10] if row < 10 else _f32_bits(x[k], -26, 43)
             for k in range(6)]
    elif cls == "F16":
        s = [F16_EDGES[row][k & 1] if row < 8
             else _f16_bits(x[k], -10, 20) | (_f16_bits(x[k] >> 16, -10, 20) << 16)
             for k in range(6)]
    elif cls == "F16FMA":
        for h in (0, 16):
            ha, hb = _f16_bits(x[0] >> h, -6, 13), _f16_bits(x[1] >> h, -6, 13)
            hc = _f16_fma_c(ha, hb, x[2] >> h)
            m = (0xFFFF << h) ^ M32
            s[0], s[1], s[2] = (s[0] & m) | (ha << h), (s[1] & m) | (hb << h), (s[2] & m) | (hc << h)
        if row < len(F16FMA_EDGES):
            s[0], s[1], s[2] = F16FMA_EDGES[row]
    elif cls in ("F64", "F64FMA"):
        if row < len(F64_EDGES) and cls == "F64":
            e = F64_EDGES[row]
            s = [*_w64(e[0]), *_w64(e[1]), *_w64(e[0])]
        elif row < len(F64FMA_EDGES):
            s = [w for v in F64FMA_EDGES[row] for w in _w64(v)]
        else:
            va, vb = _f64_small(x[0], -4, 9), _f64_small(x[1], -4, 9)
            eab = ((va >> 52) & 2047) + ((vb >> 52) & 2047) - 2046
            vc = (_f64_small(x[2], -4, 9) if cls == "F64"
                  else _f64_small(x[2], eab - 6, 13))
            s = [*_w64(va), *_w64(vb), *_w64(vc)]
    elif cls == "F64DIV":
        if row < len(F64_EDGES) - 1:
            s[0:4] = [*_w64(F64_EDGES[row + 1][0]), *_w64(F64_EDGES[row + 1][1])]
        else:
            s[0:4] = [*_w64(_f64_full(x[0], x[1], -3, 58)), *_w64(_f64_full(x[2], x[3], -3, 58))]
        s[1] &= 0x7FFFFFFF
    elif cls in ("F64R", "F64I"):
        if row < len(F64_EDGES):
            s[0:4] = [*_w64(F64_EDGES[row][0]), *_w64(F64_EDGES[row][1])]
        else:
            s[0:4] = [*_w64(_f64_full(x[0], x[1], -3, 58)), *_w64(_f64_full(x[2], x[3], -3, 58))]
        if 14 <= row < 22:
            s[1] &= 0x7FFFFFFF
        if 22 <= row < 26:
            s[0:2] = _wd(float(_sx(x[0], 32)) + 0.5)
        if cls == "F64I":
            s[2] = (x[2] % 121 - 60) & M32
    elif cls in ("DOTF16", "DOTBF16"):
        for k in range(2):
            lo, hi = x[k] % 33 - 16, (x[k] >> 8) % 33 - 16
            if cls == "DOTF16":
                s[k] = half_of(float(lo)) | (half_of(float(hi)) << 16)
            else:
                s[k] = (u32_of(float(lo)) >> 16) | (u32_of(float(hi)) & 0xFFFF0000)
        s[2] = u32_of(float(x[2] % 2001 - 1000))
    elif cls in ("FP8", "BF8", "FP4"):
        for k in range(0, 32, 8):
            code = (x[0] >> k) & 255
            if cls == "FP8" and code & 0x7F == 0x7F:
                s[0] ^= 1 << k
            if cls == "BF8" and code & 0x7C == 0x7C:
                s[0] ^= 0x40 << k
        s[1] = scale
    elif cls == "FP6":
        s = [0] * 6 if row == 0 else [M32] * 6 if row == 1 else list(x)
    elif cls == "SCALEF32":
        s[0] = SCALEF32_EDGES[row][0] if row < 6 else _f32_bits(x[0], -12, 24)
        s[1] = SCALEF32_EDGES[row][1] if row < 6 else _f32_bits(x[1], -12, 24)
        s[2] = 0x3F800000 if row < 6 else scale
    elif cls == "CMPF32":
        s[0], s[1] = CMP_F32[x[0] % 12], CMP_F32[x[1] % 12]
        if row < 12:
            s[0], s[1] = CMP_F32[row], CMP_F32[(row * 5 + 1) % 12]
    elif cls == "CMPF16":
        s[0] = CMP_F16[x[0] % 8] | (x[0] & 0xFFFF0000)
        s[1] = CMP_F16[x[1] % 8] | (x[1] & 0xFFFF0000)
    elif cls == "CMPF64":
        s[0:4] = [*_w64(CMP_F64[x[0] % 8]), *_w64(CMP_F64[x[1] % 8])]
    elif cls == "CMPINT":
        pool = (0, 1, 0x80000000, M32)
        s[0], s[1] = pool[x[0] & 3], pool[(x[0] >> 2) & 3]
        s[2], s[3] = pool[x[1] & 3], pool[(x[1] >> 2) & 3]
        if x[2] & 1:
            s[2] = s[0]
            if x[2] & 2:
                s[3] = s[1]
        if row >= 32:
            s[0], s[1] = x[0], x[3]
            if not x[2] & 1:
                s[2], s[3] = x[4], x[5]
            else:
                s[2] = s[0]
    elif cls == "CLASS32":
        s[0] = CLASS_F32[row % 10] if row < 20 else CLASS_F32[x[0] % 10]
        s[1] = 1 << row if row < 10 else x[1] & 0x3FF
    elif cls == "CLASS64":
        s[0:2] = _w64(CLASS_F64[row % 10 if row < 20 else x[0] % 10])
        s[2] = 1 << row if row < 10 else x[1] & 0x3FF
    else:  # transcendental
        k, anchor = row - 8, row < ANCHORS
        sgn = -1.0 if k & 1 else 1.0
        r32 = lambda lo, n: f32(_f32_bits(x[0], lo, n))  # noqa: E731
        r64 = lambda: f64(x[1], _f64_full(x[0], 0, -300, 600) >> 32)  # noqa: E731
        r16 = lambda lo, n: half(_f16_bits(x[0], lo, n))  # noqa: E731
        v = {
            "TEXP": lambda: float(k) if anchor else r32(-6, 12),
            "TLOG": lambda: math.ldexp(1.0, 3 * k) if anchor else abs(r32(-60, 120)),
            "TRCP": lambda: math.ldexp(sgn, 5 * k) if anchor else r32(-60, 120),
            "TSQRT": lambda: math.ldexp(1.0, 6 * k) if anchor else abs(r32(-60, 120)),
            "TSIN": lambda: 0.25 * k if anchor else r32(-6, 12),
            "TRCP64": lambda: math.ldexp(sgn, 37 * k) if anchor else r64(),
            "TSQRT64": lambda: math.ldexp(1.0, 38 * k) if anchor else abs(r64()),
            "TEXP16": lambda: float(k) if anchor else r16(-4, 7),
            "TLOG16": lambda: math.ldexp(1.0, k) if anchor else abs(r16(-10, 20)),
            "TRCP16": lambda: math.ldexp(sgn, k) if anchor else r16(-10, 20),
            "TSQRT16": lambda: (math.ldexp(1.0, 2 * int(k / 2)) if anchor
                                else abs(r16(-10, 20))),
        }[cls]()
        if cls in ("TRCP64", "TSQRT64"):
            s[0:2] = _wd(v)
        elif cls.endswith("16"):
            s[0] = half_of(v)
        else:
            s[0] = u32_of(v)
    return [w & M32 for w in s]


def alu_mbcnt(lo: int, hi: int, base: int, lane: int) -> int:
    """v_mbcnt_lo + v_mbcnt_hi: lanes below ``lane`` whose mask bit is set,
    plus the base (cro_alu_mbcnt)."""
    return (_pop(((hi << 32) | lo) & ((1 << lane) - 1)) + base) & M32


def alu_reference(form: int, s) -> tuple:
    """The two expected result words of a form on source words ``s``."""
    out = alu_forms()[form][5]([int(w) for w in s])
    if isinstance(out, tuple):
        return (int(out[0]) & M32, int(out[1]) & M32)
    return (int(out) & M32, 0)


def alu_row(seed: int, form: int, row: int) -> list:
    """cro_alu_row: six source words, two expected words."""
    s = alu_sources(seed, form, row)
    want = list(alu_reference(form, s))
    if alu_forms()[form][3] == "V1_MBCNT":
        want[0] = alu_mbcnt(s[0], s[1], s[2], row)
    if row >= checked_rows(form):  # words nothing compares are zero
        want = [0, 0]
    return s + want


def alu_table(seed: int = 0):
    """cro_alu_table as a forms x 64 x 8 uint32 array."""
    import numpy as np

    n = len(alu_forms())
    return np.array([[alu_row(seed, f, r) for r in range(ROWS)] for f in range(n)],
                    dtype=np.uint32)


# -- ctypes ------------------------------------------------------------------------------


class CroAluOpts(ctypes.Structure):
    """Mirror of ``struct CroAluOpts`` (cro_amd/hip/croalu.h)."""

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


class CroAluRecord(ctypes.Structure):
    """Mirror of ``struct CroAluRecord``: the last word is the wave's digest."""

    _fields_ = [(name, ctypes.c_uint) for name in (
        "xcc_id", "hw_id", "fail_mask", "n_bad", "first_bad", "bits_bad", "valid", "digest")]


# fields of the nested ``struct CroAluAgg`` (croalu.h), in order
ALU_AGG_FIELDS = (
    [("waves_run", ctypes.c_ulonglong), ("waves_bad", ctypes.c_ulonglong)]
    + [(f"bad_{name}", ctypes.c_ulonglong) for name in ALU_TESTS]
    + [(n, ctypes.c_int) for n in
       ("cus_seen", "xcds_seen", "simds_seen", "cus_bad", "xcd", "se", "sh", "cu", "simd")]
    + [(n, ctypes.c_uint) for n in
       ("fail_mask", "first_fail_mask", "n_bad", "first_bad", "bits_bad")]
    + [("first_bad_index", ctypes.c_longlong)]
    + [("digest", ctypes.c_uint), ("no_majority", ctypes.c_uint),
       ("digest_waves", ctypes.c_ulonglong)]
)


class CroAluResult(ctypes.Structure):
    """Mirror of ``struct CroAluResult``, the aggregate's fields written out flat."""

    _fields_ = (
        [("ok", ctypes.c_int), ("rc", ctypes.c_int), ("cus_expected", ctypes.c_int),
         ("rounds", ctypes.c_int)]
        + ALU_AGG_FIELDS
        + [("first_bad_round", ctypes.c_int), ("first_bad_record", ctypes.c_int),
           ("grid_blocks", ctypes.c_int), ("iters", ctypes.c_int),
           ("gpu_ms", ctypes.c_double), ("t_total_ms", ctypes.c_double),
           ("failed_test", ctypes.c_char * 16), ("msg", ctypes.c_char * 256)]
    )


_lib = None


def load_alu_library(required: Optional[bool] = None) -> Optional[ctypes.CDLL]:
    """Load libcroalu.so.  required=None → required iff a GPU is present;
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
                f"libcroalu.so missing at {path} — build it with "
                "`python -m cro_amd.hip.build` (hipcc --offload-arch=gfx950)"
            )
        return None
    lib = ctypes.CDLL(path)
    lib.cro_alu_run.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroAluOpts), ctypes.POINTER(CroAluResult)]
    lib.cro_alu_run.restype = ctypes.c_int
    lib.cro_alu_run_records.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroAluOpts), ctypes.POINTER(CroAluResult),
        ctypes.POINTER(CroAluRecord), ctypes.c_int]
    lib.cro_alu_run_records.restype = ctypes.c_int
    lib.cro_alu_tile.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    lib.cro_alu_tile.restype = ctypes.c_int
    _lib = lib
    return lib


def _test_index(test) -> int:
    return ALU_TESTS.index(test) if isinstance(test, str) else int(test)


def _alu_opts(grid_blocks=0, iters=0, max_rounds=0, seed=0, min_cu_fraction=0.0,
              selftest_mode=0, selftest_test=0, selftest_elem=0, selftest_bit=0,
              selftest_key=0, selftest_also=None) -> CroAluOpts:
    also = 0
    if selftest_also is not None:
        also = 1 + (form_index(selftest_also) if isinstance(selftest_also, str)
                    else int(selftest_also))
    return CroAluOpts(
        grid_blocks=int(grid_blocks), iters=int(iters), max_rounds=int(max_rounds),
        seed=int(seed) & M32, selftest_mode=int(selftest_mode),
        selftest_test=_test_index(selftest_test), selftest_bit=int(selftest_bit),
        selftest_elem=int(selftest_elem), selftest_key=int(selftest_key), selftest_also=also,
        min_cu_fraction=float(min_cu_fraction),
    )


def run_alu(device: int = 0, **opts) -> dict:
    """ALU stage: the twelve checks of croalu.h on every CU and SIMD, with the
    location of the first bad wave.  Options as ``struct CroAluOpts``; zero
    takes the library default.  A mismatch always fails (rc -38); coverage is
    reported and gates only when ``min_cu_fraction`` > 0 (rc -39).  The
    ``selftest_*`` options are for tests (``selftest_also``: a form's name or
    index)."""
    lib = load_alu_library(required=True)
    c_opts = _alu_opts(**opts)
    res = CroAluResult()
    rc = lib.cro_alu_run(device, ctypes.byref(c_opts), ctypes.byref(res))
    return _result_dict(res, rc)


def run_alu_records(device: int = 0, **opts):
    """As run_alu, and the raw per-wave records as a structured numpy array of
    rounds * grid_blocks * 4 records, round-major."""
    lib = load_alu_library(required=True)
    c_opts = _alu_opts(**opts)
    res = CroAluResult()
    return _run_with_records(CroAluRecord, c_opts, res, lambda buf, cap: (
        lib.cro_alu_run_records(device, ctypes.byref(c_opts), ctypes.byref(res), buf, cap)))


def alu_tile(device: int, form, rows):
    """One wave of the stage's own device code for ``form`` (name or index) on
    64 caller rows of six source words (cro_alu_tile).  Returns the raw result
    words, 64 x 2 uint32."""
    import numpy as np

    lib = load_alu_library(required=True)
    f = form_index(form) if isinstance(form, str) else int(form)
    buf = np.ascontiguousarray(rows, dtype=np.uint32)
    if buf.shape != (ROWS, 6):
        raise ValueError("64 rows of six source words wanted")
    out = np.zeros((ROWS, 2), dtype=np.uint32)
    rc = lib.cro_alu_tile(device, f, buf.ctypes.data, buf.nbytes, out.ctypes.data, out.nbytes)
    if rc != 0:
        raise RuntimeError(f"cro_alu_tile failed: rc={rc}")
    return out


# -- aggregation -------------------------------------------------------------------------


def aggregate_alu_records(records) -> dict:
    """Mirror of cro_alu_aggregate: the digest a strict majority of the valid
    records holds; a record that deviates (every valid record where there is
    no majority) gets the transcendental bit on a private copy; then
    probe.aggregate_wave_records."""
    import numpy as np

    copy = {name: np.array(records[name], dtype=np.uint32, copy=True)
            for name in ("xcc_id", "hw_id", "fail_mask", "n_bad", "first_bad", "bits_bad",
                         "valid", "digest")}
    valid = copy["valid"] != 0
    n_valid = int(valid.sum())
    digest, hold = 0, 0
    if n_valid:
        digest, hold = Counter(copy["digest"][valid].tolist()).most_common(1)[0]
    majority = 2 * hold > n_valid
    deviates = valid & ~(majority & (copy["digest"] == digest))
    alone = deviates & (copy["fail_mask"] == 0)
    copy["n_bad"][alone] = 1
    copy["first_bad"][alone] = M32
    copy["bits_bad"][alone] = (copy["digest"][alone] ^ np.uint32(digest)) if majority else 0
    copy["fail_mask"][deviates] |= np.uint32(1 << TRANS)
    out, fail_mask, _ = aggregate_wave_records(copy, ALU_TESTS)
    out["fail_mask"] = fail_mask
    out["digest"] = int(digest) if majority and n_valid else 0
    out["no_majority"] = int(bool(n_valid) and not majority)
    out["digest_waves"] = int(hold) if majority else 0
    return out


def alu_test_name(fail_mask: int) -> str:
    """The lowest failing check of a fail mask (cro_alu_test_name)."""
    for bit, name in enumerate(ALU_TESTS):
        if fail_mask & (1 << bit):
            return name
    return ""


def describe_first_bad(first_bad: int) -> str:
    """"form v_mul_hi_u32 row 3 lane 17" for a failure's first_bad; a wave
    whose only fault is its digest has none."""
    if first_bad == M32:
        return "digest differs"
    d = decode_first_bad(first_bad)
    forms = alu_forms()
    label = forms[d["form"]][2] if d["form"] < len(forms) else str(d["form"])
    return f"form {label} row {d['row']} lane {d['lane']}"
