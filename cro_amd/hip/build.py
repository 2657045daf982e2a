"""Build the gfx950 HIP probe extension in-tree.

Usage: ``python -m cro_amd.hip.build``  (also driven by __graft_entry__.build)

hipcc cross-compiles for gfx950 without a GPU present; the resulting .so
lives next to the source so it travels with repo snapshots.
"""

from __future__ import annotations

import os
import subprocess
import sys

HIP_DIR = os.path.dirname(os.path.abspath(__file__))
AGENT_DIR = os.path.join(os.path.dirname(HIP_DIR), "agent")
SRC = os.path.join(HIP_DIR, "probe.hip")
# quick probe + deep (data-integrity) probe + compute-coverage stage, one
# shared library: ALL_SRCS, rebuilt when any of ALL_HEADERS changes
SRCS = [SRC, os.path.join(HIP_DIR, "integrity.hip")]
HEADERS = [os.path.join(HIP_DIR, "croprobe.h"), os.path.join(HIP_DIR, "cropattern.h")]
# compute-coverage stage: one more source and header of the same library
# (listed apart: tests/test_probe_integrity.py pins what SRCS and HEADERS hold)
COVERAGE_SRC = os.path.join(HIP_DIR, "coverage.hip")
COVERAGE_HEADER = os.path.join(HIP_DIR, "crocoverage.h")
# what the three sources share and nothing else includes: host plumbing and
# the wave-level matrix code
INTERNAL_HEADERS = [os.path.join(HIP_DIR, "crohost.h"), os.path.join(HIP_DIR, "cromfma.h")]
# the deep probe's host-only pieces (integrity.hip includes it; listed apart
# for the same reason)
INTEGRITY_HEADER = os.path.join(HIP_DIR, "crointegrity.h")
ALL_SRCS = SRCS + [COVERAGE_SRC]
ALL_HEADERS = HEADERS + [COVERAGE_HEADER, INTEGRITY_HEADER] + INTERNAL_HEADERS
OUT = os.path.join(HIP_DIR, "libcroprobe.so")
# scrub-on-detach stage: a library of its own (the probe library's lists
# above are pinned by its tests), with its own staleness check
SCRUB_SRC = os.path.join(HIP_DIR, "scrub.hip")
SCRUB_HEADERS = [
    os.path.join(HIP_DIR, "croscrub.h"),
    os.path.join(HIP_DIR, "croscrubplan.h"),
    os.path.join(HIP_DIR, "crohost.h"),
    INTEGRITY_HEADER,  # for PatternReport
    HEADERS[1],  # cropattern.h, which crointegrity.h includes
]
SCRUB_OUT = os.path.join(HIP_DIR, "libcroscrub.so")
# LDS scrub stage: again a library of its own (the scrub library's list above
# is pinned by its tests too)
LDS_SCRUB_SRC = os.path.join(HIP_DIR, "ldsscrub.hip")
LDS_SCRUB_HEADERS = [
    os.path.join(HIP_DIR, "croldsscrub.h"),
    os.path.join(HIP_DIR, "crohost.h"),
    COVERAGE_HEADER,  # for cro_cov_cu_key and cro_cov_decode
]
LDS_SCRUB_OUT = os.path.join(HIP_DIR, "libcroldsscrub.so")
# register scrub stage: a library of its own once more (the LDS scrub
# library's list above is pinned by its tests too)
REG_SCRUB_SRC = os.path.join(HIP_DIR, "regscrub.hip")
REG_SCRUB_HEADERS = [
    os.path.join(HIP_DIR, "croregscrub.h"),
    os.path.join(HIP_DIR, "crohost.h"),
    COVERAGE_HEADER,  # for cro_cov_decode
]
REG_SCRUB_OUT = os.path.join(HIP_DIR, "libcroregscrub.so")
# matrix-format probe stage: a library of its own as well (the probe
# library's lists above are pinned by its tests); cromfma.h for the f32
# result maps
FORMATS_SRC = os.path.join(HIP_DIR, "formats.hip")
FORMATS_HEADERS = [
    os.path.join(HIP_DIR, "croformats.h"),
    os.path.join(HIP_DIR, "crohost.h"),
    os.path.join(HIP_DIR, "cromfma.h"),
    COVERAGE_HEADER,  # for cro_cov_cu_key, cro_cov_decode and the LCG
]
FORMATS_OUT = os.path.join(HIP_DIR, "libcroformats.so")
# coherence probe stage (atomics and cross-CU visibility): a library of its
# own too (the lists above are pinned by their tests)
COHERENCE_SRC = os.path.join(HIP_DIR, "coherence.hip")
COHERENCE_HEADERS = [
    os.path.join(HIP_DIR, "crocoherence.h"),
    os.path.join(HIP_DIR, "crohost.h"),
    COVERAGE_HEADER,  # for cro_cov_cu_key and cro_cov_decode
]
COHERENCE_OUT = os.path.join(HIP_DIR, "libcrocoherence.so")
# data-movement probe stage (cross-lane, transposed LDS reads, LDS-DMA): a
# library of its own as well (the lists above are pinned by their tests)
MOVEMENT_SRC = os.path.join(HIP_DIR, "movement.hip")
MOVEMENT_HEADERS = [
    os.path.join(HIP_DIR, "cromovement.h"),
    os.path.join(HIP_DIR, "crohost.h"),
    COVERAGE_HEADER,  # for cro_cov_cu_key and cro_cov_decode
]
MOVEMENT_OUT = os.path.join(HIP_DIR, "libcromovement.so")
# ALU probe stage (vector and scalar ALUs, transcendental consensus): a
# library of its own as well; croformats.h for the narrow formats' code tables
ALU_SRC = os.path.join(HIP_DIR, "alu.hip")
ALU_HEADERS = [
    os.path.join(HIP_DIR, "croalu.h"),
    os.path.join(HIP_DIR, "crohost.h"),
    os.path.join(HIP_DIR, "croformats.h"),
    COVERAGE_HEADER,  # for cro_cov_cu_key, cro_cov_decode and the aggregation core
]
ALU_OUT = os.path.join(HIP_DIR, "libcroalu.so")
AGENT_SRC = os.path.join(AGENT_DIR, "croagent.cpp")
AGENT_OUT = os.path.join(AGENT_DIR, "croagent")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the library's device compile flags, named once: tests/test_probe_quick.py
# produces assembly with them to look at the code the library really runs
DEVICE_FLAGS = ["--offload-arch=gfx950", "-O3"]


def _stale(out: str, inputs) -> bool:
    """True when ``out`` is missing or older than any of its inputs."""
    if not os.path.exists(out):
        return True
    built = os.path.getmtime(out)
    return any(os.path.getmtime(path) > built for path in inputs)


def build(force: bool = False) -> str:
    if force or _stale(OUT, ALL_SRCS + ALL_HEADERS):
        subprocess.run(
            [HIPCC, *DEVICE_FLAGS, "-fPIC", "-shared", *ALL_SRCS, "-o", OUT],
            check=True,
        )
    build_agent(force=force)
    return OUT


def build_scrub(force: bool = False) -> str:
    """libcroscrub.so: the scrub-on-detach stage (scrub.hip)."""
    if force or _stale(SCRUB_OUT, [SCRUB_SRC] + SCRUB_HEADERS):
        subprocess.run(
            [HIPCC, *DEVICE_FLAGS, "-fPIC", "-shared", SCRUB_SRC, "-o", SCRUB_OUT],
            check=True,
        )
    return SCRUB_OUT


def build_lds_scrub(force: bool = False) -> str:
    """libcroldsscrub.so: the LDS scrub stage (ldsscrub.hip)."""
    if force or _stale(LDS_SCRUB_OUT, [LDS_SCRUB_SRC] + LDS_SCRUB_HEADERS):
        subprocess.run(
            [HIPCC, *DEVICE_FLAGS, "-fPIC", "-shared", LDS_SCRUB_SRC, "-o", LDS_SCRUB_OUT],
            check=True,
        )
    return LDS_SCRUB_OUT


def build_reg_scrub(force: bool = False) -> str:
    """libcroregscrub.so: the register scrub stage (regscrub.hip)."""
    if force or _stale(REG_SCRUB_OUT, [REG_SCRUB_SRC] + REG_SCRUB_HEADERS):
        subprocess.run(
            [HIPCC, *DEVICE_FLAGS, "-fPIC", "-shared", REG_SCRUB_SRC, "-o", REG_SCRUB_OUT],
            check=True,
        )
    return REG_SCRUB_OUT


def build_formats(force: bool = False) -> str:
    """libcroformats.so: the matrix-format probe stage (formats.hip)."""
    if force or _stale(FORMATS_OUT, [FORMATS_SRC] + FORMATS_HEADERS):
        subprocess.run(
            [HIPCC, *DEVICE_FLAGS, "-fPIC", "-shared", FORMATS_SRC, "-o", FORMATS_OUT],
            check=True,
        )
    return FORMATS_OUT


def build_coherence(force: bool = False) -> str:
    """libcrocoherence.so: the coherence probe stage (coherence.hip)."""
    if force or _stale(COHERENCE_OUT, [COHERENCE_SRC] + COHERENCE_HEADERS):
        subprocess.run(
            [HIPCC, *DEVICE_FLAGS, "-fPIC", "-shared", COHERENCE_SRC, "-o", COHERENCE_OUT],
            check=True,
        )
    return COHERENCE_OUT


def build_movement(force: bool = False) -> str:
    """libcromovement.so: the data-movement probe stage (movement.hip)."""
    if force or _stale(MOVEMENT_OUT, [MOVEMENT_SRC] + MOVEMENT_HEADERS):
        subprocess.run(
            [HIPCC, *DEVICE_FLAGS, "-fPIC", "-shared", MOVEMENT_SRC, "-o", MOVEMENT_OUT],
            check=True,
        )
    return MOVEMENT_OUT


def build_alu(force: bool = False) -> str:
    """libcroalu.so: the ALU probe stage (alu.hip)."""
    if force or _stale(ALU_OUT, [ALU_SRC] + ALU_HEADERS):
        subprocess.run(
            [HIPCC, *DEVICE_FLAGS, "-fPIC", "-shared", ALU_SRC, "-o", ALU_OUT],
            check=True,
        )
    return ALU_OUT


def build_agent(force: bool = False) -> str:
    """croagent: the native node-agent CLI (links libcroprobe; loads
    libcroscrub.so, libcroldsscrub.so, libcroregscrub.so, libcroformats.so and
    libcrocoherence.so at run time, so those libraries are no inputs here, and
    neither are croscrub.h, croldsscrub.h, croregscrub.h, croformats.h and
    crocoherence.h, which the agent
    includes: the input list below is pinned by
    tests/test_probe_compute.py.  A --force build, which is what `make build`
    does, picks up a change of those headers)."""
    if not force and not _stale(AGENT_OUT, [AGENT_SRC, HEADERS[0], COVERAGE_HEADER, OUT]):
        return AGENT_OUT
    subprocess.run(
        [
            HIPCC,
            "--offload-arch=gfx950",
            "-O2",
            AGENT_SRC,
            f"-L{HIP_DIR}",
            "-lcroprobe",
            f"-Wl,-rpath,{HIP_DIR}",
            "-Wl,-rpath,$ORIGIN/../hip",
            "-o",
            AGENT_OUT,
        ],
        check=True,
    )
    return AGENT_OUT


if __name__ == "__main__":
    path = build(force="--force" in sys.argv)
    print(path)
    print(AGENT_OUT)
    print(build_scrub(force="--force" in sys.argv))
    print(build_lds_scrub(force="--force" in sys.argv))
    print(build_formats(force="--force" in sys.argv))
    print(build_coherence(force="--force" in sys.argv))
    print(build_movement(force="--force" in sys.argv))
    print(build_alu(force="--force" in sys.argv))
    print(build_reg_scrub(force="--force" in sys.argv))
