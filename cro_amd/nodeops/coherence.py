"""ctypes wrapper for the coherence probe stage (cro_amd/hip/coherence.hip →
libcrocoherence.so): exact checks of the atomic units in L2 / memory and in
every CU's LDS and of cross-CU, cross-XCD visibility, with fault location, and
the numpy mirrors of what cro_amd/hip/crocoherence.h decides on the host: every
lane's contributions, a workgroup's totals (closed forms and the fold over its
lanes), the expected tally lines, the payload hash and the aggregation.

The loader takes ``required=False`` for callers that only ask whether the
stage is available; running the stage without the compiled library is an
error, never a silent pass.  What the stage covers and what it does not (LDS
packed adds, system-scope and fine-grained memory, the sc1 hand-off forms,
buffer-addressed atomics, rates) is in crocoherence.h.
"""

from __future__ import annotations

import ctypes
import os
from typing import Optional

from .probe import _gpu_present, _result_dict, decode_location

_LIB_PATH = os.path.join(os.path.dirname(__file__), "..", "hip", "libcrocoherence.so")

COHERENCE_TESTS = ("add_u32", "add_u64", "add_f32", "add_f64", "pk_add_f16", "pk_add_bf16",
                   "minmax", "bitwise", "ticket", "cas", "lds_rmw", "visibility")
TALLY_TESTS = 8
RC_MISMATCH = -34
RC_COVERAGE = -35
MAX_GRID = 1024
MAX_ITERS = 64
UNIT_WORDS = 32
SLOTS = 18
XCD_IDS = 16
SUBS = 16
GROUP = 64
PAYLOAD = 64
LEVELS = ("workgroup", "xcd", "device")
SLOT_NAMES = ("add_u32", "add_u64", "add_f32", "add_f64", "pk_add_f16", "pk_add_bf16",
              "min_u32", "max_u32", "min_i32", "max_i32", "min_f64", "max_f64",
              "and_u32", "or_u32", "xor_u32", "and_u64", "or_u64", "xor_u64")
F64_FAR = 1 << 60
_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF
_K = 2097143


def _test_index(test) -> int:
    return COHERENCE_TESTS.index(test) if isinstance(test, str) else int(test)


def slot_test(slot: int) -> int:
    """The check a slot of a unit belongs to (cro_coh_slot_test)."""
    return slot if slot < 6 else 6 if slot < 12 else 7


class CroCoherenceOpts(ctypes.Structure):
    """Mirror of ``struct CroCoherenceOpts`` (cro_amd/hip/crocoherence.h)."""

    _fields_ = [
        ("grid_blocks", ctypes.c_int),
        ("iters", ctypes.c_int),
        ("max_rounds", ctypes.c_int),
        ("seed", ctypes.c_uint),
        ("selftest_mode", ctypes.c_int),
        ("selftest_test", ctypes.c_int),
        ("selftest_bit", ctypes.c_int),
        ("selftest_key", ctypes.c_uint),
        ("min_cu_fraction", ctypes.c_double),
    ]


RECORD_FIELDS = ("xcc_id", "hw_id", "fail_mask", "n_bad", "first_bad", "bits_bad", "valid",
                 "block", "vis_pairs", "vis_bad", "vis_stale", "vis_first_block",
                 "vis_first_dword", "vis_bits", "preread", "epoch")


class CroCoherenceRecord(ctypes.Structure):
    """Mirror of ``struct CroCoherenceRecord`` (cro_amd/hip/crocoherence.h)."""

    _fields_ = [(name, ctypes.c_uint) for name in RECORD_FIELDS]


# fields of the nested ``struct CroCoherenceAgg`` (crocoherence.h), in order
COHERENCE_AGG_FIELDS = (
    [("waves_run", ctypes.c_ulonglong), ("waves_bad", ctypes.c_ulonglong)]
    + [(f"bad_{name}", ctypes.c_ulonglong) for name in COHERENCE_TESTS]
    + [(n, ctypes.c_ulonglong) for n in
       ("pairs_checked", "pairs_expected", "vis_bad", "vis_stale", "tally_got", "tally_want")]
    + [("first_bad_index", ctypes.c_longlong)]
    + [(n, ctypes.c_int) for n in
       ("cus_seen", "xcds_seen", "simds_seen", "cus_bad", "xcd", "se", "sh", "cu", "simd")]
    + [(n, ctypes.c_uint) for n in
       ("fail_mask", "first_fail_mask", "n_bad", "first_bad", "bits_bad")]
    + [(n, ctypes.c_int) for n in
       ("tally_level", "tally_slot", "tally_unit", "tally_epoch", "bad_block",
        "ticket_slot", "ticket_epoch")]
    + [(n, ctypes.c_uint) for n in ("ticket_seen", "ticket_owner", "reserved")]
)


class CroCoherenceResult(ctypes.Structure):
    """Mirror of ``struct CroCoherenceResult`` (cro_amd/hip/crocoherence.h),
    with the nested aggregate's fields written out flat."""

    _fields_ = (
        [
            ("ok", ctypes.c_int),
            ("rc", ctypes.c_int),
            ("cus_expected", ctypes.c_int),
            ("rounds", ctypes.c_int),
        ]
        + COHERENCE_AGG_FIELDS
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


def load_coherence_library(required: Optional[bool] = None) -> Optional[ctypes.CDLL]:
    """Load libcrocoherence.so.  required=None → required iff a GPU is present;
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
                f"libcrocoherence.so missing at {path} — build it with "
                "`python -m cro_amd.hip.build` (hipcc --offload-arch=gfx950)"
            )
        return None
    lib = ctypes.CDLL(path)
    lib.cro_coherence_run.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroCoherenceOpts), ctypes.POINTER(CroCoherenceResult),
    ]
    lib.cro_coherence_run.restype = ctypes.c_int
    lib.cro_coherence_run_records.argtypes = [
        ctypes.c_int, ctypes.POINTER(CroCoherenceOpts), ctypes.POINTER(CroCoherenceResult),
        ctypes.POINTER(CroCoherenceRecord), ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong,
    ]
    lib.cro_coherence_run_records.restype = ctypes.c_int
    _lib = lib
    return lib


def _coherence_opts(grid_blocks=0, iters=0, max_rounds=0, seed=0, min_cu_fraction=0.0,
                    selftest_mode=0, selftest_test=0, selftest_bit=0,
                    selftest_key=0) -> CroCoherenceOpts:
    return CroCoherenceOpts(
        grid_blocks=int(grid_blocks), iters=int(iters), max_rounds=int(max_rounds),
        seed=int(seed) & _M32, selftest_mode=int(selftest_mode),
        selftest_test=_test_index(selftest_test), selftest_bit=int(selftest_bit),
        selftest_key=int(selftest_key), min_cu_fraction=float(min_cu_fraction),
    )


def run_coherence(device: int = 0, **opts) -> dict:
    """Coherence stage: the twelve checks of crocoherence.h on every CU.
    Options as ``struct CroCoherenceOpts``; zero takes the library default.  A
    mismatch always fails (rc -34); coverage is reported and gates only when
    ``min_cu_fraction`` > 0 (rc -35).  The ``selftest_*`` options are for
    tests."""
    lib = load_coherence_library(required=True)
    c_opts = _coherence_opts(**opts)
    res = CroCoherenceResult()
    rc = lib.cro_coherence_run(device, ctypes.byref(c_opts), ctypes.byref(res))
    return _result_dict(res, rc)


def run_coherence_records(device: int = 0, **opts):
    """As run_coherence, and returns of the last round the raw per-wave
    records (a structured numpy array of iters * grid_blocks * 4 records,
    launch-major) and the tally units as downloaded (uint64, iters x units x
    32)."""
    import numpy as np

    lib = load_coherence_library(required=True)
    c_opts = _coherence_opts(**opts)
    res = CroCoherenceResult()
    blocks = c_opts.grid_blocks or MAX_GRID
    iters = c_opts.iters or MAX_ITERS
    cap = blocks * 4 * iters
    buf = (CroCoherenceRecord * cap)()
    unit_cap = coherence_units(blocks) * UNIT_WORDS * iters
    units = np.zeros(unit_cap, dtype=np.uint64)
    rc = lib.cro_coherence_run_records(device, ctypes.byref(c_opts), ctypes.byref(res), buf, cap,
                                       units.ctypes.data, unit_cap)
    out = _result_dict(res, rc)
    grid, iters = out["grid_blocks"], out["iters"]
    n = min(iters * grid * 4, cap)
    dtype = np.dtype([(name, np.uint32) for name in RECORD_FIELDS])
    records = np.frombuffer(buf, dtype=dtype, count=cap)[:n].copy()
    per = coherence_units(grid) * UNIT_WORDS if grid else 0
    units = units[: per * iters].reshape(iters, -1, UNIT_WORDS) if per else units[:0]
    return out, records, units


# -- numpy mirrors of crocoherence.h ---------------------------------------------------


def coherence_units(grid: int) -> int:
    return grid + XCD_IDS * SUBS + SUBS


def sub_slot(block: int) -> int:
    return (block >> 3) & 15


def xcd_unit(grid: int, xcc_id: int, block: int) -> int:
    return grid + (xcc_id & 15) * SUBS + sub_slot(block)


def dev_unit(grid: int, block: int) -> int:
    return grid + XCD_IDS * SUBS + sub_slot(block)


def unit_level(grid: int, unit: int):
    """(level, what the line names: block, XCD or device sub-slot)."""
    if unit < grid:
        return 0, unit
    if unit < grid + XCD_IDS * SUBS:
        return 1, (unit - grid) // SUBS
    return 2, unit - grid - XCD_IDS * SUBS


def _lcg(s: int) -> int:
    return (s * 1664525 + 1013904223) & _M32


def coherence_salt(seed: int, epoch: int) -> int:
    return _lcg(_lcg((seed ^ (epoch * 0x9E3779B9)) & _M32))


def pk_rule(kind: int, wide: int):
    """(P, M) of a packed add: kind 0 f16, 1 bf16; wide 0 the workgroup line."""
    if kind == 0:
        return (64, 8) if wide else (4, 16)
    return (256, 4) if wide else (16, 8)


def drop_tid(test, block: int) -> int:
    idx = _test_index(test)
    return block % 64 if idx == 4 else block % 256 if idx == 5 else 0


def lane_values(block: int, salt: int, wide: int) -> dict:
    """Every lane's contributions to a unit, as int64 / uint64 arrays of 256
    (packed adds: 0 where a lane takes no part, with the mask ``pk*_on``)."""
    import numpy as np

    tid = np.arange(256, dtype=np.int64)
    g = block * 256 + tid
    bit = np.int64(1) << (tid & 31)
    m_and = (((block + 1) * 0x9E3779B1) & _M32) ^ salt
    m_or = (((block + 1) * 0x85EBCA6B) & _M32) ^ salt
    neg = (tid & 3) == 3
    out = {
        "add_u32": (g * 2654435761 + (salt | 1)) & _M32,
        "add_u64": ((g + 1).astype(np.uint64) * np.uint64(0x39E3779B1)),
        "add_f32": np.where(neg, -1, 1) * (1 + tid + (block & 255)),
        "add_f64": np.where(neg, -1, 1) * (g + 1) * _K,
        "mm32": ((g & 1) << 31) | (g * 8 + 5),
        "mmf64": np.where(g & 1, -1, 1) * (g + 1) * _K,
        "and_u32": ~(m_and & bit) & _M32,
        "or_u32": m_or & bit,
        "xor_u32": (((g + 1) << 13) | ((g + 1) >> 19)) & _M32,
        "and_u64": ~((m_and & bit).astype(np.uint64) << np.uint64(20)),
        "or_u64": (m_or & bit).astype(np.uint64) << np.uint64(24),
        "xor_u64": ((g + 1).astype(np.uint64) << np.uint64(32))
        | ((~(g + 1)) & _M32).astype(np.uint64),
    }
    for kind, name in ((0, "f16"), (1, "bf16")):
        p, m = pk_rule(kind, wide)
        on = (tid % p) == (block % p)
        lo = 1 + (g // p) % m
        out[f"{name}_on"] = on
        out[f"{name}_lo"] = np.where(on, lo, 0)
        out[f"{name}_hi"] = np.where(on, m + 1 - lo, 0)
    return out


def totals_init() -> dict:
    return {"add32": 0, "add64": 0, "f32": 0, "f64": 0, "f16_lo": 0, "f16_hi": 0,
            "bf16_lo": 0, "bf16_hi": 0, "min_u": _M32, "max_u": 0, "min_i": 0x7FFFFFFF,
            "max_i": -0x80000000, "min_f": F64_FAR, "max_f": -F64_FAR, "and32": _M32, "or32": 0,
            "xor32": 0, "and64": _M64, "or64": 0, "xor64": 0}


def _signed32(x: int) -> int:
    return x - (1 << 32) if x & 0x80000000 else x


def block_totals_brute(block: int, salt: int, wide: int, skip=None, skip_tid=None) -> dict:
    """A workgroup's totals by folding every lane in turn; ``skip`` leaves the
    operations of that check out for lane ``skip_tid`` (self-test mode 2)."""
    import numpy as np

    v = lane_values(block, salt, wide)
    skip = None if skip is None else _test_index(skip)
    keep = np.ones(256, dtype=bool)
    if skip is not None:
        keep[drop_tid(skip, block) if skip_tid is None else skip_tid] = False

    def lanes(test):
        return keep if skip == test else np.ones(256, dtype=bool)

    t = totals_init()
    t["add32"] = int(v["add_u32"][lanes(0)].sum()) & _M32
    t["add64"] = int(sum(int(x) for x in v["add_u64"][lanes(1)])) & _M64
    t["f32"] = int(v["add_f32"][lanes(2)].sum())
    t["f64"] = int(v["add_f64"][lanes(3)].sum())
    t["f16_lo"], t["f16_hi"] = int(v["f16_lo"][lanes(4)].sum()), int(v["f16_hi"][lanes(4)].sum())
    t["bf16_lo"] = int(v["bf16_lo"][lanes(5)].sum())
    t["bf16_hi"] = int(v["bf16_hi"][lanes(5)].sum())
    mm = [int(x) for x in v["mm32"][lanes(6)]]
    mf = [int(x) for x in v["mmf64"][lanes(6)]]
    t["min_u"], t["max_u"] = min(mm + [_M32]), max(mm + [0])
    t["min_i"] = min([_signed32(x) for x in mm] + [0x7FFFFFFF])
    t["max_i"] = max([_signed32(x) for x in mm] + [-0x80000000])
    t["min_f"], t["max_f"] = min(mf + [F64_FAR]), max(mf + [-F64_FAR])
    for name, key, op, start in (("and32", "and_u32", "and", _M32), ("or32", "or_u32", "or", 0),
                                 ("xor32", "xor_u32", "xor", 0), ("and64", "and_u64", "and", _M64),
                                 ("or64", "or_u64", "or", 0), ("xor64", "xor_u64", "xor", 0)):
        acc = start
        for x in v[key][lanes(7)]:
            x = int(x)
            acc = acc & x if op == "and" else acc | x if op == "or" else acc ^ x
        t[name] = acc
    return t


def _xor_upto(n: int) -> int:
    return (n, 1, n + 1, 0)[n & 3]


def _cycle_sum(q0: int, n: int, m: int) -> int:
    full, rest = divmod(n, m)
    return full * (m * (m + 1) // 2) + sum(1 + (q0 + j) % m for j in range(rest))


def block_totals(block: int, salt: int, wide: int) -> dict:
    """The same totals in closed form (cro_coh_block_totals)."""
    base = block * 256
    t = totals_init()
    t["add32"] = (2654435761 * (256 * base + 32640) + 256 * (salt | 1)) & _M32
    t["add64"] = (0x39E3779B1 * (256 * base + 32896)) & _M64
    t["f32"] = 16256 + 128 * (block & 255)
    t["f64"] = _K * (128 * base + 16256)
    for kind, name in ((0, "f16"), (1, "bf16")):
        p, m = pk_rule(kind, wide)
        n = 256 // p
        lo = _cycle_sum(n * block, n, m)
        t[f"{name}_lo"], t[f"{name}_hi"] = lo, n * (m + 1) - lo
    t["min_u"] = base * 8 + 5
    t["max_u"] = 0x80000000 | ((base + 255) * 8 + 5)
    t["min_i"] = _signed32(0x80000000 | ((base + 1) * 8 + 5))
    t["max_i"] = (base + 254) * 8 + 5
    t["min_f"] = -(base + 256) * _K
    t["max_f"] = (base + 255) * _K
    xr = _xor_upto(base + 256) ^ _xor_upto(base)
    m_and = (((block + 1) * 0x9E3779B1) & _M32) ^ salt
    m_or = (((block + 1) * 0x85EBCA6B) & _M32) ^ salt
    t["and32"] = ~m_and & _M32
    t["or32"] = m_or
    t["xor32"] = ((xr << 13) | (xr >> 19)) & _M32
    t["and64"] = ~(m_and << 20) & _M64
    t["or64"] = m_or << 24
    t["xor64"] = (xr << 32) | xr
    return t


def totals_fold(acc: dict, b: dict) -> None:
    acc["add32"] = (acc["add32"] + b["add32"]) & _M32
    acc["add64"] = (acc["add64"] + b["add64"]) & _M64
    for k in ("f32", "f64", "f16_lo", "f16_hi", "bf16_lo", "bf16_hi"):
        acc[k] += b[k]
    for k in ("min_u", "min_i", "min_f"):
        acc[k] = min(acc[k], b[k])
    for k in ("max_u", "max_i", "max_f"):
        acc[k] = max(acc[k], b[k])
    for k in ("and32", "and64"):
        acc[k] &= b[k]
    for k in ("or32", "or64"):
        acc[k] |= b[k]
    for k in ("xor32", "xor64"):
        acc[k] ^= b[k]


def encode_totals(t: dict):
    """The 32 words of a unit that holds these totals (cro_coh_encode)."""
    import numpy as np

    def f16(v):
        return int(np.array(v, dtype=np.float16).view(np.uint16))

    def f32(v):
        return int(np.array(v, dtype=np.float32).view(np.uint32))

    def f64(v):
        return int(np.array(v, dtype=np.float64).view(np.uint64))

    w = [0] * UNIT_WORDS
    w[0], w[1], w[2], w[3] = t["add32"], t["add64"], f32(t["f32"]), f64(t["f64"])
    w[4] = f16(t["f16_lo"]) | (f16(t["f16_hi"]) << 16)
    w[5] = (f32(t["bf16_lo"]) >> 16) | (f32(t["bf16_hi"]) & 0xFFFF0000)
    w[6], w[7] = t["min_u"], t["max_u"]
    w[8], w[9] = t["min_i"] & _M32, t["max_i"] & _M32
    w[10], w[11] = f64(t["min_f"]), f64(t["max_f"])
    w[12], w[13], w[14] = t["and32"], t["or32"], t["xor32"]
    w[15], w[16], w[17] = t["and64"], t["or64"], t["xor64"]
    return np.array(w, dtype=np.uint64)


def initial_units(grid: int):
    import numpy as np

    return np.tile(encode_totals(totals_init()), (coherence_units(grid), 1))


def expected_units(grid: int, seed: int, epoch: int, xcc_of_block, drop=None):
    """What every unit holds after the launch of ``epoch`` (uint64, units x
    32): cro_coh_expected_units.  ``drop`` = (block or blocks, check) leaves
    one lane's operations of that check out in those workgroups, as self-test
    mode 2 does."""
    import numpy as np

    salt = coherence_salt(seed & _M32, epoch)
    units = np.zeros((coherence_units(grid), UNIT_WORDS), dtype=np.uint64)
    shared = [totals_init() for _ in range(XCD_IDS * SUBS + SUBS)]
    dropped = set()
    if drop is not None:
        dropped = {drop[0]} if isinstance(drop[0], int) else set(drop[0])
    for b in range(grid):
        if b in dropped:
            own = block_totals_brute(b, salt, 0, skip=drop[1])
            wide = block_totals_brute(b, salt, 1, skip=drop[1])
        else:
            own, wide = block_totals(b, salt, 0), block_totals(b, salt, 1)
        units[b] = encode_totals(own)
        totals_fold(shared[xcd_unit(0, int(xcc_of_block[b]), b)], wide)
        totals_fold(shared[dev_unit(0, b)], wide)
    for u, t in enumerate(shared):
        units[grid + u] = encode_totals(t)
    return units


def payload_value(seed: int, epoch: int, block: int, idx: int) -> int:
    """cro_coh_payload."""
    s = coherence_salt(seed & _M32, epoch) ^ (((block * PAYLOAD + idx) * 0x9E3779B9) & _M32)
    return _lcg(_lcg(s))


def coherence_test_name(fail_mask: int) -> str:
    """The lowest failing check of a fail mask (cro_coh_test_name)."""
    for bit, name in enumerate(COHERENCE_TESTS):
        if fail_mask & (1 << bit):
            return name
    return ""


def _agg_clear() -> dict:
    out = {"waves_run": 0, "waves_bad": 0}
    out.update({f"bad_{name}": 0 for name in COHERENCE_TESTS})
    out.update(pairs_checked=0, pairs_expected=0, vis_bad=0, vis_stale=0, tally_got=0,
               tally_want=0, first_bad_index=-1, cus_seen=0, xcds_seen=0, simds_seen=0,
               cus_bad=0, xcd=-1, se=-1, sh=-1, cu=-1, simd=-1, fail_mask=0, first_fail_mask=0,
               n_bad=0, first_bad=_M32, bits_bad=0, tally_level=-1, tally_slot=-1,
               tally_unit=-1, tally_epoch=-1, bad_block=-1, ticket_slot=-1, ticket_epoch=-1,
               ticket_seen=0, ticket_owner=0)
    return out


def _place(out: dict, rec, with_simd: bool) -> None:
    loc = decode_location(int(rec["xcc_id"]), int(rec["hw_id"]))
    out.update({k: int(loc[k]) for k in ("xcd", "se", "sh", "cu")})
    out["simd"] = int(loc["simd"]) if with_simd else -1


def aggregate_coherence_records(records, grid: int, launches: int) -> dict:
    """numpy mirror of cro_coherence_aggregate over a structured record array,
    launch-major (launch, block, wave)."""
    import numpy as np

    out = _agg_clear()
    n = launches * grid * 4
    valid = np.asarray(records["valid"])[:n] != 0
    xcc = np.asarray(records["xcc_id"])[:n].astype(np.int64)
    hw = np.asarray(records["hw_id"])[:n].astype(np.int64)
    mask = np.where(valid, np.asarray(records["fail_mask"])[:n].astype(np.int64), 0)
    keys = ((xcc & 0xF) << 16) | (hw & 0xFF00)
    bad = mask != 0
    out["waves_run"] = int(valid.sum())
    out["waves_bad"] = int(bad.sum())
    for bit in range(TALLY_TESTS, len(COHERENCE_TESTS)):
        out[f"bad_{COHERENCE_TESTS[bit]}"] = int(((mask >> bit) & 1).sum())
    out["cus_seen"] = int(np.unique(keys[valid]).size)
    out["xcds_seen"] = int(np.unique(xcc[valid] & 0xF).size)
    out["simds_seen"] = int(np.unique((keys * 4 + ((hw >> 4) & 3))[valid]).size)
    out["cus_bad"] = int(np.unique(keys[bad]).size)
    out["vis_bad"] = int(np.asarray(records["vis_bad"])[:n][valid].sum())
    out["vis_stale"] = int(np.asarray(records["vis_stale"])[:n][valid].sum())
    out["fail_mask"] = int(np.bitwise_or.reduce(mask)) if n else 0
    pairs = np.where(valid, np.asarray(records["vis_pairs"])[:n].astype(np.int64), 0)
    pairs = pairs.reshape(launches, grid, 4)
    whole = valid.reshape(launches, grid, 4)
    for launch in range(launches):
        for g0 in range(0, grid, GROUP):
            m = min(GROUP, grid - g0)
            got = int(pairs[launch, g0:g0 + m].sum())
            want = m * (m - 1) // 2
            out["pairs_checked"] += got
            out["pairs_expected"] += want
            if whole[launch, g0:g0 + m].all() and got != want:
                out["fail_mask"] |= 1 << 11
                out["bad_visibility"] += 1
    if bad.any():
        first = int(np.flatnonzero(bad)[0])
        rec = {k: records[k][first] for k in RECORD_FIELDS}
        _place(out, rec, True)
        out.update(first_bad_index=first, first_fail_mask=int(rec["fail_mask"]),
                   n_bad=int(rec["n_bad"]), first_bad=int(rec["first_bad"]),
                   bits_bad=int(rec["bits_bad"]))
        if coherence_test_name(int(rec["fail_mask"])) == "visibility":
            out["bad_block"] = int(np.int32(rec["vis_first_block"]))
        else:
            out["bad_block"] = int(rec["block"])
    return out


def check_tallies(got, want, grid: int, epoch: int, launch_records, out: dict) -> int:
    """cro_coh_check_tallies: ``got`` and ``want`` are units x 32 uint64."""
    import numpy as np

    got = np.asarray(got, dtype=np.uint64).reshape(-1, UNIT_WORDS)[:, :SLOTS]
    want = np.asarray(want, dtype=np.uint64).reshape(-1, UNIT_WORDS)[:, :SLOTS]
    bad_units, bad_slots = np.nonzero(got != want)
    for u, s in zip(bad_units.tolist(), bad_slots.tolist()):
        test = slot_test(s)
        out[f"bad_{COHERENCE_TESTS[test]}"] += 1
        out["fail_mask"] |= 1 << test
        if out["tally_level"] >= 0:
            continue
        level, name = unit_level(grid, u)
        out.update(tally_level=level, tally_unit=name, tally_slot=s, tally_epoch=epoch,
                   tally_got=int(got[u, s]), tally_want=int(want[u, s]))
        if level == 0:
            out["bad_block"] = name
            rec = {k: launch_records[k][name * 4] for k in RECORD_FIELDS}
            if rec["valid"]:
                _place(out, rec, False)
        elif level == 1:
            out["xcd"] = name
    return len(bad_units)


def check_tickets(seen, owner, grid: int, epoch: int, want_of_0: int, launch_records,
                  out: dict) -> int:
    """cro_coh_check_tickets."""
    import numpy as np

    n = grid * 256
    seen = np.asarray(seen)[:n].astype(np.int64)
    want = np.ones(n, dtype=np.int64)
    want[0] = want_of_0
    bad = np.flatnonzero(seen != want)
    if bad.size == 0:
        return 0
    out["bad_ticket"] += int(bad.size)
    out["fail_mask"] |= 1 << 8
    if out["ticket_slot"] < 0:
        t = int(bad[0])
        who = int(owner[t])
        out.update(ticket_slot=t, ticket_epoch=epoch, ticket_seen=int(seen[t]), ticket_owner=who)
        if who < n and out["tally_level"] < 0:
            out["bad_block"] = who >> 8
            rec = {k: launch_records[k][who >> 6] for k in RECORD_FIELDS}
            if rec["valid"]:
                _place(out, rec, True)
    return int(bad.size)


def check_words(words, grid: int, out: dict) -> int:
    """cro_coh_check_words."""
    n_bad = 0
    for g0 in range(0, grid, GROUP):
        m = min(GROUP, grid - g0)
        if int(words[g0 // GROUP]) != (1 << m) - 1:
            n_bad += 1
            out["bad_visibility"] += 1
            out["fail_mask"] |= 1 << 11
    return n_bad


def host_findings() -> dict:
    """An empty aggregate for check_tallies / check_tickets / check_words."""
    return _agg_clear()


def merge_findings(out: dict, host: dict) -> None:
    """cro_coh_agg_merge."""
    for name in COHERENCE_TESTS:
        out[f"bad_{name}"] += host[f"bad_{name}"]
    wave_mask = out["fail_mask"]
    out["fail_mask"] |= host["fail_mask"]
    for k in ("tally_got", "tally_want", "tally_level", "tally_slot", "tally_unit", "tally_epoch",
              "ticket_slot", "ticket_epoch", "ticket_seen", "ticket_owner"):
        out[k] = host[k]
    host_low = host["fail_mask"] & -host["fail_mask"]
    wave_low = wave_mask & -wave_mask
    if (host_low & 0x1FF) and (not wave_low or host_low < wave_low):
        out.update(first_bad_index=-1, first_fail_mask=0)
        for k in ("xcd", "se", "sh", "cu", "simd", "bad_block"):
            out[k] = host[k]
