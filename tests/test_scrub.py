"""CPU tests of the scrub-on-detach feature: the two C structs against their
Python mirrors and the allocation plan (through small host programs built with
the host C++ compiler — no HIP, no GPU), the numpy reference, the controller's
scrub phase, the operator flags, the exec path, the agent's subcommand on a
machine without a GPU, and the build of the library."""

import argparse
import ctypes
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from cro_amd.api.v1alpha1.types import ComposableResource, Event
from cro_amd.nodeops import scrub as scrub_mod
from cro_amd.nodeops.amdgpu import DrainInProgress, ScrubFailed
from tests.conftest import make_node, make_resource

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(REPO, "cro_amd", "hip")
AGENT = os.path.join(REPO, "cro_amd", "agent", "croagent")
MIB = 1 << 20
GIB = 1 << 30
FLOOR = 2 * MIB
NONE = (1 << 64) - 1


def _host_cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    pytest.fail("no host C++ compiler (c++/g++/clang++) on PATH")


def _build(tmp_path, name, source, extra=()):
    src = tmp_path / f"{name}.cpp"
    src.write_text(source)
    exe = tmp_path / name
    subprocess.run(
        [_host_cxx(), "-std=c++17", "-O1", *extra, f"-I{HIP_DIR}", str(src), "-o", str(exe)],
        check=True, capture_output=True, text=True,
    )
    return str(exe)


def _run(exe, *args):
    return subprocess.run([exe, *map(str, args)], check=True, capture_output=True,
                          text=True).stdout


# -- struct mirrors ----------------------------------------------------------------

MIRRORS = {"CroScrubOpts": scrub_mod.CroScrubOpts, "CroScrubResult": scrub_mod.CroScrubResult}


def _layout_source():
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "croscrub.h"', "int main() {"]
    for cname, mirror in MIRRORS.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for field, _ in mirror._fields_:
            lines.append(
                f'  printf("{cname} {field} %zu %zu\\n", offsetof({cname}, {field}), '
                f"sizeof((({cname}*)0)->{field}));"
            )
    lines += ["  return 0;", "}"]
    return "\n".join(lines)


def test_struct_mirrors_match_the_header(tmp_path):
    out = _run(_build(tmp_path, "scrub_layout", _layout_source()))
    seen = set()
    for line in out.splitlines():
        parts = line.split()
        mirror = MIRRORS[parts[0]]
        if parts[1] == "sizeof":
            assert ctypes.sizeof(mirror) == int(parts[2]), line
        else:
            desc = getattr(mirror, parts[1])
            assert (desc.offset, desc.size) == (int(parts[2]), int(parts[3])), line
        seen.add((parts[0], parts[1]))
    assert len(seen) == sum(len(m._fields_) + 1 for m in MIRRORS.values())


def test_struct_mirrors_have_no_holes():
    """A hole would be a field of the header that the mirror lacks."""
    for mirror in MIRRORS.values():
        end = 0
        for field, _ in mirror._fields_:
            desc = getattr(mirror, field)
            assert desc.offset == end, (mirror.__name__, field)
            end = desc.offset + desc.size
        assert end == ctypes.sizeof(mirror)


# -- croscrubplan.h ------------------------------------------------------------------

PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "croscrubplan.h"
using namespace croscrub;
static unsigned long long num(const char* s) { return strtoull(s, nullptr, 10); }
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const char* cmd = argv[1];
  if (!strcmp(cmd, "target") && argc == 5) {  // free reserve max
    printf("%llu\n", (unsigned long long)target_bytes(num(argv[2]), atoll(argv[3]), atoll(argv[4])));
    return 0;
  }
  if (!strcmp(cmd, "chunk") && argc == 3) {
    printf("%llu\n", (unsigned long long)normalise_chunk(atoll(argv[2])));
    return 0;
  }
  if (!strcmp(cmd, "plan") && argc == 6) {  // target chunk_option allocator param
    const uint64_t target = num(argv[2]);
    const uint64_t chunk = normalise_chunk(atoll(argv[3]));
    const uint64_t param = num(argv[5]);
    uint64_t used = 0, n = 0;
    const PlanStats s = acquire(target, chunk, [&](uint64_t bytes) {
      ++n;
      bool ok = true;
      if (!strcmp(argv[4], "cap")) ok = used + bytes <= param;  // grants until capacity
      if (!strcmp(argv[4], "nth")) ok = n != param;             // refuses the n-th request
      if (ok) used += bytes;
      printf("%llu %d\n", (unsigned long long)bytes, ok ? 1 : 0);
      return ok;
    });
    printf("stats %llu %llu %llu %llu\n", (unsigned long long)s.granted_bytes,
           (unsigned long long)s.requests, (unsigned long long)s.refusals,
           (unsigned long long)s.chunks);
    return 0;
  }
  if (!strcmp(cmd, "locate") && argc >= 4) {  // span_word chunk_words...
    ChunkList list;
    for (int i = 3; i < argc; ++i) list.add(num(argv[i]));
    const ChunkList::Pos pos = list.locate(num(argv[2]));
    printf("%llu %llu %llu %llu %llu\n", (unsigned long long)pos.chunk,
           (unsigned long long)pos.word, (unsigned long long)list.count(),
           (unsigned long long)list.span_words(), (unsigned long long)list.base(pos.chunk));
    return 0;
  }
  return 2;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("scrubplan"), "scrubplan_main", PLAN_MAIN)


def _plan(exe, target, chunk, allocator="grant", param=0):
    """(requests as (bytes, granted) pairs, stats dict) of one plan."""
    lines = _run(exe, "plan", target, chunk, allocator, param).splitlines()
    requests = [(int(a), bool(int(b))) for a, b in (l.split() for l in lines[:-1])]
    granted, n, refusals, chunks = (int(v) for v in lines[-1].split()[1:])
    stats = {"granted": granted, "requests": n, "refusals": refusals, "chunks": chunks}
    assert n == len(requests)
    assert refusals == sum(not ok for _, ok in requests)
    assert chunks == sum(ok for _, ok in requests)
    assert granted == sum(b for b, ok in requests if ok)
    return requests, stats


def _check_plan_properties(requests, target, chunk):
    """What holds for every plan, whatever the allocator answers."""
    left, limit = target, chunk
    for i, (ask, ok) in enumerate(requests):
        assert ask % 256 == 0 and ask > 0
        assert ask <= left, "never more than the remaining target"
        assert ask <= limit, "after a refusal at s, every later request <= s/2"
        if ok:
            left -= ask
        else:
            limit = (ask // 2) & ~255
            if ask <= FLOOR:
                assert i == len(requests) - 1, "a refusal at or below the floor ends the plan"
    last_ask, last_ok = requests[-1]
    assert left < 256 or (not last_ok and last_ask <= FLOOR), "stopped early"


def test_plan_exact_sequences(plan_exe):
    t = 5 * MIB + 768
    reqs, stats = _plan(plan_exe, t, 2 * MIB)
    assert reqs == [(2 * MIB, True), (2 * MIB, True), (MIB + 768, True)]
    assert stats["granted"] == t
    # bytes past the last whole 256 are not asked for by the plan itself:
    # target_bytes rounds down before (below)
    reqs, _ = _plan(plan_exe, 8 * MIB, 4 * MIB, "nth", 2)
    assert reqs == [(4 * MIB, True), (4 * MIB, False), (2 * MIB, True), (2 * MIB, True)]
    # the remainder below the floor is asked for once, as it is
    reqs, stats = _plan(plan_exe, 4 * MIB + 512, 4 * MIB, "nth", 2)
    assert reqs == [(4 * MIB, True), (512, False)]
    assert stats["granted"] == 4 * MIB
    # capacity 7 MiB: 4 ok, 4 refused, 2 ok, 2 refused (at the floor: stop)
    reqs, stats = _plan(plan_exe, 16 * MIB, 4 * MIB, "cap", 7 * MIB)
    assert reqs == [(4 * MIB, True), (4 * MIB, False), (2 * MIB, True), (2 * MIB, False)]
    assert stats["granted"] == 6 * MIB
    # a refusal above the floor halves to below it; that size is still tried
    reqs, _ = _plan(plan_exe, 9 * MIB, 3 * MIB, "cap", 5 * MIB)
    assert reqs == [(3 * MIB, True), (3 * MIB, False), (MIB + MIB // 2, True),
                    (MIB + MIB // 2, False)]
    # nothing granted at all
    reqs, stats = _plan(plan_exe, 8 * MIB, 8 * MIB, "cap", 0)
    assert [r[0] for r in reqs] == [8 * MIB, 4 * MIB, 2 * MIB]
    assert stats["granted"] == 0 and stats["chunks"] == 0
    # a target below one allocation unit asks for nothing
    assert _plan(plan_exe, 255, MIB)[0] == []


def _issue_bound(target, chunk):
    return target // chunk + math.log2(chunk / FLOOR) + 2


PLAN_CASES = [
    (5 * MIB + 768, 2 * MIB), (64 * MIB, 4 * MIB), (GIB + 256, 0), (7 * GIB + 3 * MIB, GIB),
    (96 * MIB + 4096, 32 * MIB), (256, 2 * MIB), (3 * MIB, 2 * MIB + 256),
]


@pytest.mark.parametrize("target,chunk_opt", PLAN_CASES)
def test_plan_properties_when_everything_is_granted(plan_exe, target, chunk_opt):
    chunk = int(_run(plan_exe, "chunk", chunk_opt))
    reqs, stats = _plan(plan_exe, target, chunk_opt)
    _check_plan_properties(reqs, target, chunk)
    assert stats["granted"] == target and stats["refusals"] == 0
    assert stats["requests"] == -(-target // chunk)
    assert stats["requests"] <= _issue_bound(target, chunk)


@pytest.mark.parametrize("target,chunk_opt", PLAN_CASES)
@pytest.mark.parametrize("nth", [1, 2, 3])
def test_plan_properties_when_the_nth_request_is_refused(plan_exe, target, chunk_opt, nth):
    chunk = int(_run(plan_exe, "chunk", chunk_opt))
    reqs, stats = _plan(plan_exe, target, chunk_opt, "nth", nth)
    _check_plan_properties(reqs, target, chunk)
    if len(reqs) < nth:  # the plan was over before the n-th request
        assert stats["refusals"] == 0 and stats["granted"] == target
        return
    assert stats["refusals"] == 1
    refused = reqs[nth - 1][0]
    if refused > FLOOR:
        assert stats["granted"] == target  # a refusal is not a failure
        # one refusal, and the rest of the target in halves: twice the
        # requests that were still to come, at most
        before = nth - 1
        assert stats["requests"] <= before + 1 + 2 * (-(-(target - before * chunk) // chunk)) + 1
    else:
        assert len(reqs) == nth and stats["granted"] == sum(b for b, _ in reqs[:-1])


CAPACITIES = [0, 256, FLOOR - 256, FLOOR, 3 * MIB, 7 * MIB, 37 * MIB + 512, 64 * MIB, GIB - 256,
              GIB + 5 * MIB]


@pytest.mark.parametrize("capacity", CAPACITIES)
@pytest.mark.parametrize("target,chunk_opt", PLAN_CASES)
def test_plan_properties_when_capacity_runs_out(plan_exe, target, chunk_opt, capacity):
    """The request count: the issue puts it at target/chunk + log2(chunk/floor)
    + 2.  That holds whenever at most one request is granted after the first
    refusal (asserted here for those cases, with a power-of-two chunk so that
    the logarithm counts the halvings, and above when nothing is refused).  For
    a general capacity the stated plan asks twice per halved size when that
    size is granted once (granted, asked again, refused), e.g. chunk 1 GiB and
    capacity 1 GiB - 256 B: 1 refusal at 1 GiB, then a grant and a refusal at
    each of 512 MiB .. 2 MiB = 19 requests against a bound of 12.  What the
    plan as stated can guarantee is 2 x log2 in place of log2, asserted for
    every case."""
    chunk = int(_run(plan_exe, "chunk", chunk_opt))
    reqs, stats = _plan(plan_exe, target, chunk_opt, "cap", capacity)
    if not reqs:
        assert target < 256
        return
    _check_plan_properties(reqs, target, chunk)
    assert stats["granted"] <= min(target, capacity)
    if capacity >= target:
        assert stats["granted"] == target and stats["refusals"] == 0
    else:
        # what is left of the capacity is less than the last size refused
        assert capacity - stats["granted"] < reqs[-1][0] or target - stats["granted"] < 256
    levels = max(math.ceil(math.log2(chunk / FLOOR)), 0)
    assert stats["requests"] <= target // chunk + 2 * levels + 3
    first_refusal = [ok for _, ok in reqs].index(False) if stats["refusals"] else len(reqs)
    grants_after_a_refusal = sum(ok for _, ok in reqs[first_refusal:])
    if grants_after_a_refusal <= 1 and chunk >= FLOOR and chunk & (chunk - 1) == 0:
        assert stats["requests"] <= _issue_bound(target, chunk)


def test_target_bytes(plan_exe):
    def target(free, reserve, max_bytes):
        return int(_run(plan_exe, "target", free, reserve, max_bytes))

    assert target(10 * GIB, 0, 0) == 10 * GIB - 256 * MIB  # default reserve
    assert target(10 * GIB, GIB, 0) == 9 * GIB  # a larger reserve is honoured
    assert target(10 * GIB, MIB, 0) == 10 * GIB - 256 * MIB  # a smaller one is raised
    assert target(10 * GIB + 300, 0, 0) == 10 * GIB - 256 * MIB + 256  # whole 256 B
    assert target(10 * GIB, 0, 96 * MIB + 4096) == 96 * MIB + 4096
    assert target(10 * GIB, 0, 5 * MIB + 1023) == 5 * MIB + 768
    assert target(10 * GIB, 0, 100 * GIB) == 10 * GIB - 256 * MIB  # the cap only lowers
    # free <= reserve: nothing to scrub (the stage then reports rc -1 with
    # "nothing to scrub"; tests/test_scrub_gpu.py)
    assert target(256 * MIB, 0, 0) == 0
    assert target(100 * MIB, 0, 0) == 0
    assert target(GIB, 2 * GIB, 0) == 0
    assert target(256 * MIB + 255, 0, 0) == 0


def test_normalise_chunk(plan_exe):
    chunk = lambda v: int(_run(plan_exe, "chunk", v))  # noqa: E731
    assert chunk(0) == GIB and chunk(-5) == GIB and chunk(GIB + 1) == GIB and chunk(GIB) == GIB
    assert chunk(32 * MIB) == 32 * MIB and chunk(MIB + 300) == MIB + 256 and chunk(100) == 256


@pytest.mark.parametrize("word,want", [
    (0, (0, 0)), (1023, (0, 1023)), (1024, (1, 0)), (1024 + 511, (1, 511)), (1536, (2, 0)),
    (1536 + 63, (2, 63)),
])
def test_chunk_list_locates_span_words(plan_exe, word, want):
    out = [int(v) for v in _run(plan_exe, "locate", word, 1024, 512, 64).split()]
    assert tuple(out[:2]) == want
    assert out[2:4] == [3, 1600]
    assert out[4] == [0, 1024, 1536][want[0]]


def test_plan_program_under_host_sanitizers(tmp_path):
    """The same stand-alone host program, built with ASan and UBSan."""
    try:
        exe = _build(tmp_path, "scrubplan_san", PLAN_MAIN,
                     extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    except subprocess.CalledProcessError as exc:
        pytest.skip(f"host compiler cannot build with sanitizers: {exc.stderr[-200:]}")
    for args in (("plan", 7 * GIB + 3 * MIB, GIB, "cap", GIB - 256),
                 ("plan", 8 * MIB, 4 * MIB, "nth", 2),
                 ("plan", 255, MIB, "grant", 0),
                 ("locate", 1599, 1024, 512, 64),
                 ("target", 256 * MIB, 0, 0)):
        proc = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr
        assert "runtime error" not in proc.stderr and "Sanitizer" not in proc.stderr


# -- numpy reference -----------------------------------------------------------------


def test_scrub_report_reference():
    clean = np.zeros(10, dtype=np.uint32)
    assert scrub_mod.scrub_report(clean, 0) == {"n_bad": 0, "first_bad": NONE, "bits_bad": 0}
    words = np.full(10, 0xDEADBEEF, dtype=np.uint32)
    assert scrub_mod.scrub_report(words, 0xDEADBEEF, 77)["n_bad"] == 0
    words[3] ^= 0x10
    words[7] ^= 0x80000001
    assert scrub_mod.scrub_report(words, 0xDEADBEEF) == {
        "n_bad": 2, "first_bad": 3, "bits_bad": 0x80000011}
    base = (1 << 40) + 5
    assert scrub_mod.scrub_report(words, 0xDEADBEEF, base)["first_bad"] == base + 3
    assert scrub_mod.scrub_report(words, 0) == {
        "n_bad": 10, "first_bad": 0, "bits_bad": 0xDEADBEEF | 0xDEADBEFF | 0x5EADBEEE}
    assert scrub_mod.scrub_report(np.zeros(0, dtype=np.uint32), 0)["n_bad"] == 0


def test_load_scrub_library_is_loud_only_where_required(monkeypatch, tmp_path):
    monkeypatch.setattr(scrub_mod, "_lib", None)
    monkeypatch.setattr(scrub_mod, "_LIB_PATH", str(tmp_path / "libcroscrub.so"))
    assert scrub_mod.load_scrub_library(required=False) is None
    with pytest.raises(RuntimeError, match="libcroscrub.so missing"):
        scrub_mod.load_scrub_library(required=True)
    monkeypatch.setattr(scrub_mod, "_gpu_present", lambda: True)
    with pytest.raises(RuntimeError, match="on a GPU node"):
        scrub_mod.load_scrub_library()


# -- controller ----------------------------------------------------------------------

OK_RESULT = {
    "ok": True, "rc": 0, "vram_total": 288 * GIB, "bytes_scrubbed": 3 * GIB + 512 * MIB,
    "bytes_verified": 3 * GIB + 512 * MIB, "fraction": 3.5 / 288, "dirty_words_before": 1234,
    "n_bad": 0, "first_bad_byte": NONE, "bits_bad": 0, "t_total_ms": 41.6, "msg": "ok",
}
RESIDUE_RESULT = dict(OK_RESULT, ok=False, rc=-40, n_bad=3, first_bad_byte=4096,
                      bits_bad=0x00010001, msg="residue after scrub: 3 bad words")


class _Scrub:
    """A fake ops.scrub that answers from a list (the last answer repeats)."""

    def __init__(self, world, answers):
        self.world, self.answers, self.calls = world, list(answers), 0
        world.ops.scrub = self

    def __call__(self, node, device_id):
        self.calls += 1
        self.world.ops.calls.append(("scrub", node, device_id))
        answer = self.answers[min(self.calls, len(self.answers)) - 1]
        return dict(answer) if answer is not None else None


def _online(world, name="gpu-1", **kw):
    make_node(world.client, "node0")
    world.client.create(make_resource(name, **kw))
    world.resource_rec.reconcile(name)
    world.resource_rec.reconcile(name)
    assert world.client.get(ComposableResource, name).status.state == "Online"


def _start_detach(world, name="gpu-1"):
    world.client.delete(ComposableResource, name)
    world.resource_rec.reconcile(name)  # Online → Detaching
    assert world.client.get(ComposableResource, name).status.state == "Detaching"


def _reasons(world):
    return [e.reason for e in sorted(world.client.list(Event), key=lambda e: e.first_seen)]


def _events(world, reason):
    return [e for e in world.client.list(Event) if e.reason == reason]


def _counter(metrics, reason):
    return metrics.scrub_failures_total.labels(reason=reason)._value.get()


def test_scrub_runs_after_load_check_and_taint_and_before_drain(mock_world, monkeypatch):
    from cro_amd.controllers import composableresource as ctrl

    _online(mock_world)
    _Scrub(mock_world, [OK_RESULT])
    real_taint = ctrl.taints.create_device_taint

    def taint(client, resource):
        mock_world.ops.calls.append(("taint", resource.metadata.name))
        return real_taint(client, resource)

    monkeypatch.setattr(ctrl.taints, "create_device_taint", taint)
    _start_detach(mock_world)
    mock_world.ops.calls.clear()
    mock_world.resource_rec.reconcile("gpu-1")
    order = [c[0] for c in mock_world.ops.calls]
    assert order[:4] == ["check_no_loads", "taint", "scrub", "drain"], order
    device_id = mock_world.ops.calls[3][2]
    assert mock_world.ops.calls[2] == ("scrub", "node0", device_id)


def test_scrub_success_event_and_metrics(mock_world):
    _online(mock_world)
    scrub = _Scrub(mock_world, [OK_RESULT])
    metrics = mock_world.resource_rec.metrics
    bytes_before = metrics.scrub_bytes_total._value.get()
    _start_detach(mock_world)
    device_id = mock_world.client.get(ComposableResource, "gpu-1").status.device_id
    mock_world.resource_rec.reconcile("gpu-1")
    assert scrub.calls == 1
    (event,) = _events(mock_world, "Scrubbed")
    assert event.type == "Normal"
    assert event.message == (
        f"scrubbed 3.50 GiB (1.2 % of VRAM) of device {device_id}, verified; "
        "1234 dirty words found before; 42 ms"
    )
    assert metrics.scrub_bytes_total._value.get() - bytes_before == 3 * GIB + 512 * MIB
    assert _reasons(mock_world) == ["AttachStarted", "FabricAttached", "Online", "DetachStarted",
                                    "Scrubbed", "Detached"]


def test_scrub_once_across_fabric_waits(mock_world):
    from cro_amd.fabric.mock import MockFabricConfig

    _online(mock_world)
    scrub = _Scrub(mock_world, [OK_RESULT])
    mock_world.fabric.config = MockFabricConfig(asynchronous=True, detach_latency=0.05)
    _start_detach(mock_world)
    res = mock_world.resource_rec.reconcile("gpu-1")  # scrub, drain, fabric: waiting
    assert res.requeue_after is not None
    assert mock_world.client.get(ComposableResource, "gpu-1").status.state == "Detaching"
    mock_world.resource_rec.reconcile("gpu-1")
    import time

    time.sleep(0.06)
    for _ in range(3):
        mock_world.resource_rec.reconcile("gpu-1")
    assert mock_world.client.try_get(ComposableResource, "gpu-1") is None
    assert scrub.calls == 1
    assert len(_events(mock_world, "Scrubbed")) == 1


def test_scrub_once_when_drain_is_in_progress_first(mock_world):
    _online(mock_world)
    scrub = _Scrub(mock_world, [OK_RESULT])
    real_drain = mock_world.ops.drain
    state = {"n": 0}

    def drain(node, device_id):
        state["n"] += 1
        if state["n"] <= 2:
            raise DrainInProgress("still unloading")
        return real_drain(node, device_id)

    mock_world.ops.drain = drain
    _start_detach(mock_world)
    for _ in range(2):
        res = mock_world.resource_rec.reconcile("gpu-1")
        assert res.requeue_after is not None
    mock_world.resource_rec.reconcile("gpu-1")
    assert state["n"] == 3 and scrub.calls == 1
    assert mock_world.client.get(ComposableResource, "gpu-1").status.state == "Deleting"
    # the bookkeeping is dropped with the detach
    assert mock_world.resource_rec._scrub_done == {}


def test_failed_scrub_blocks_the_detach_and_is_tried_again(mock_world):
    _online(mock_world)
    scrub = _Scrub(mock_world, [RESIDUE_RESULT, OK_RESULT])
    metrics = mock_world.resource_rec.metrics
    before = _counter(metrics, "residue")
    removed = []
    real_remove = mock_world.fabric.remove_resource
    mock_world.fabric.remove_resource = lambda r: (removed.append(r.metadata.name),
                                                   real_remove(r))[1]
    _start_detach(mock_world)
    mock_world.ops.calls.clear()
    with pytest.raises(ScrubFailed):
        mock_world.resource_rec.reconcile("gpu-1")
    assert "drain" not in [c[0] for c in mock_world.ops.calls] and removed == []
    got = mock_world.client.get(ComposableResource, "gpu-1")
    assert got.status.state == "Detaching" and got.status.device_id != ""
    assert got.status.error.startswith(f"scrub of device {got.status.device_id} failed: residue "
                                       "first_bad_byte=4096 bits_bad=0x00010001 n_bad=3 ")
    (event,) = _events(mock_world, "ScrubFailed")
    assert event.type == "Warning" and event.message == got.status.error
    assert _counter(metrics, "residue") - before == 1
    assert _events(mock_world, "Scrubbed") == []
    # the next reconcile scrubs again, passes, and the detach completes
    mock_world.resource_rec.reconcile("gpu-1")
    assert scrub.calls == 2
    assert "drain" in [c[0] for c in mock_world.ops.calls] and removed == ["gpu-1"]
    assert mock_world.client.get(ComposableResource, "gpu-1").status.state == "Deleting"
    assert len(_events(mock_world, "Scrubbed")) == 1


@pytest.mark.parametrize("result,reason", [
    (RESIDUE_RESULT, "residue"),
    (dict(OK_RESULT, ok=False, rc=-41, msg="scrubbed fraction below floor"), "fraction"),
    (dict(ok=False, rc=-1, msg="hipMalloc failed"), "error"),
    (dict(ok=False, rc=1, msg="croagent scrub failed"), "error"),
])
def test_failure_reasons(mock_world, result, reason):
    _online(mock_world)
    _Scrub(mock_world, [result])
    metrics = mock_world.resource_rec.metrics
    before = _counter(metrics, reason)
    _start_detach(mock_world)
    with pytest.raises(ScrubFailed, match=f"failed: {reason} "):
        mock_world.resource_rec.reconcile("gpu-1")
    assert _counter(metrics, reason) - before == 1


def test_scrub_that_raises_is_a_failed_scrub(mock_world):
    _online(mock_world)

    def scrub(node, device_id):
        raise RuntimeError("libcroscrub.so missing")

    mock_world.ops.scrub = scrub
    before = _counter(mock_world.resource_rec.metrics, "error")
    _start_detach(mock_world)
    with pytest.raises(ScrubFailed, match="failed: error .*RuntimeError: libcroscrub.so missing"):
        mock_world.resource_rec.reconcile("gpu-1")
    assert _counter(mock_world.resource_rec.metrics, "error") - before == 1
    assert "drain" not in [c[0] for c in mock_world.ops.calls]
    assert len(_events(mock_world, "ScrubFailed")) == 1


def test_failed_scrub_with_force_detach_warns_and_detaches(mock_world):
    _online(mock_world, force_detach=True)
    scrub = _Scrub(mock_world, [RESIDUE_RESULT])
    metrics = mock_world.resource_rec.metrics
    before = _counter(metrics, "residue")
    _start_detach(mock_world)
    for _ in range(3):
        mock_world.resource_rec.reconcile("gpu-1")
    assert mock_world.client.try_get(ComposableResource, "gpu-1") is None
    assert scrub.calls == 1
    (event,) = _events(mock_world, "ScrubFailed")
    assert event.type == "Warning" and "residue" in event.message
    assert event.message.endswith("force_detach: detaching anyway")
    assert _counter(metrics, "residue") - before == 1
    reasons = _reasons(mock_world)
    assert "Detached" in reasons and "Scrubbed" not in reasons and "ReconcileError" not in reasons


@pytest.mark.parametrize("install", [False, True])
def test_no_scrub_leaves_the_event_trail_unchanged(mock_world, install):
    """ops.scrub answering None (the default of every NodeOps) is today's detach."""
    _online(mock_world)
    if install:
        _Scrub(mock_world, [None])
    else:
        assert mock_world.ops.scrub("node0", "GPU-x") is None
    _start_detach(mock_world)
    for _ in range(3):
        mock_world.resource_rec.reconcile("gpu-1")
    assert mock_world.client.try_get(ComposableResource, "gpu-1") is None
    assert _reasons(mock_world) == ["AttachStarted", "FabricAttached", "Online", "DetachStarted",
                                    "Detached"]


def test_default_scrub_of_every_node_ops_is_none():
    from cro_amd.nodeops.amdgpu import AmdNodeOps, MockNodeOps, NodeOps
    from cro_amd.nodeops.cxl import CxlNodeOps
    from cro_amd.nodeops.execs import MockNodeExec

    assert NodeOps().scrub("n", "d") is None
    assert MockNodeOps().scrub("n", "d") is None
    assert CxlNodeOps(MockNodeExec(), destructive=False).scrub("n", "d") is None
    assert AmdNodeOps(MockNodeExec(), destructive=False).scrub("n", "d") is None


def test_amd_node_ops_scrub_hook():
    from cro_amd.nodeops.amdgpu import AmdNodeOps
    from cro_amd.nodeops.execs import MockNodeExec

    seen = []
    ops = AmdNodeOps(MockNodeExec(), destructive=False,
                     scrub_fn=lambda gpu: seen.append(gpu) or {"ok": True})
    gpu = object()
    ops.find_gpu = lambda node, device_id: gpu if device_id == "GPU-here" else None
    assert ops.scrub("n", "GPU-gone") is None and seen == []  # no longer enumerable
    assert ops.scrub("n", "GPU-here") == {"ok": True} and seen == [gpu]


def test_scrub_metrics_are_registered_and_reset():
    from prometheus_client import REGISTRY

    from cro_amd.metrics import Metrics

    names = ("cro_scrub_failures_total", "cro_scrub_seconds", "cro_scrub_bytes_total")

    def registered():
        return {n for n in names if n in REGISTRY._names_to_collectors}

    Metrics()
    assert registered() == set(names)
    Metrics._reset_for_tests()
    try:
        assert registered() == set()
    finally:
        Metrics()  # as every other test expects it
    assert registered() == set(names)


# -- entry point ---------------------------------------------------------------------

SCRUB_ENV = ("CRO_SCRUB_ON_DETACH", "CRO_SCRUB_MAX_MIB", "CRO_SCRUB_RESERVE_MIB",
             "CRO_SCRUB_MIN_FRACTION")


def _parse(argv, monkeypatch, env=None):
    from cro_amd.cmd.main import add_scrub_arguments

    for name in SCRUB_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    p = argparse.ArgumentParser()
    add_scrub_arguments(p)
    return p.parse_args(argv)


def test_scrub_flags_default_off(monkeypatch):
    from cro_amd.cmd.main import select_scrub_fn

    args = _parse([], monkeypatch)
    assert (args.scrub_on_detach, args.scrub_max_mib, args.scrub_reserve_mib,
            args.scrub_min_fraction) == ("off", 0, 0, 0.0)
    assert select_scrub_fn(args) is None


def test_scrub_flags_and_environment(monkeypatch):
    from cro_amd.cmd import main as main_mod

    args = _parse(["--scrub-on-detach", "on", "--scrub-max-mib", "1024", "--scrub-reserve-mib",
                   "512", "--scrub-min-fraction", "0.9"], monkeypatch)
    assert (args.scrub_on_detach, args.scrub_max_mib, args.scrub_reserve_mib,
            args.scrub_min_fraction) == ("on", 1024, 512, 0.9)
    env = {"CRO_SCRUB_ON_DETACH": "on", "CRO_SCRUB_MAX_MIB": "64", "CRO_SCRUB_RESERVE_MIB": "300",
           "CRO_SCRUB_MIN_FRACTION": "0.5"}
    args = _parse([], monkeypatch, env)
    assert (args.scrub_on_detach, args.scrub_max_mib, args.scrub_reserve_mib,
            args.scrub_min_fraction) == ("on", 64, 300, 0.5)
    # the flag wins over the environment
    args = _parse(["--scrub-on-detach", "off", "--scrub-max-mib", "8"], monkeypatch, env)
    assert args.scrub_on_detach == "off" and args.scrub_max_mib == 8
    assert main_mod.select_scrub_fn(args) is None
    with pytest.raises(SystemExit):
        _parse(["--scrub-on-detach", "maybe"], monkeypatch)

    made = {}
    monkeypatch.setattr(scrub_mod, "make_scrub_fn", lambda **kw: made.update(kw) or "hook")
    args = _parse(["--scrub-on-detach", "on", "--scrub-max-mib", "3", "--scrub-min-fraction",
                   "0.25"], monkeypatch)
    assert main_mod.select_scrub_fn(args) == "hook"
    assert made == {"max_bytes": 3 * MIB, "reserve_bytes": 0, "min_fraction": 0.25}


def test_make_scrub_fn_runs_on_the_devices_ordinal(monkeypatch):
    calls = []
    monkeypatch.setattr(scrub_mod, "hip_device_for_bdf", lambda bdf: {"0000:5a:00.0": 3}.get(bdf))
    monkeypatch.setattr(scrub_mod, "run_scrub", lambda dev, **kw: calls.append((dev, kw)) or {})

    class Gpu:
        pci_bdf = "0000:5a:00.0"

    fn = scrub_mod.make_scrub_fn(max_bytes=5, reserve_bytes=6, min_fraction=0.5)
    fn(Gpu())
    Gpu.pci_bdf = "0000:ff:00.0"
    scrub_mod.make_scrub_fn()(Gpu())
    assert calls == [
        (3, {"max_bytes": 5, "reserve_bytes": 6, "min_fraction": 0.5}),
        (0, {"max_bytes": 0, "reserve_bytes": 0, "min_fraction": 0.0}),
    ]


# -- exec path -----------------------------------------------------------------------


class _Exec:
    def __init__(self, rc=0, out="", err=""):
        self.answer, self.calls = (rc, out, err), []

    def run(self, node, argv, timeout=None):
        self.calls.append((node, list(argv), timeout))
        return self.answer


class _Gpu:
    pci_bdf = "0000:5a:00.0"


def test_scrub_via_exec_argv():
    ok = json.dumps({"ok": True, "rc": 0, "bytes_scrubbed": 64 * MIB})
    execer = _Exec(0, ok + "\n")
    assert scrub_mod.scrub_via_exec(execer, "node7", _Gpu()) == json.loads(ok)
    assert execer.calls == [("node7", ["croagent", "scrub", "--bdf", "0000:5a:00.0"], 300)]
    execer = _Exec(0, ok)
    scrub_mod.scrub_via_exec(execer, "node7", _Gpu(), argv_prefix=["chroot", "/run/amdgpu-driver"],
                             max_mib=1024, reserve_mib=512, min_fraction=0.9)
    assert execer.calls[0][1] == [
        "chroot", "/run/amdgpu-driver", "croagent", "scrub", "--bdf", "0000:5a:00.0",
        "--max-mib", "1024", "--reserve-mib", "512", "--min-fraction", "0.9"]
    execer = _Exec(0, ok)
    prefixes = iter([[], ["chroot", "/x"]])
    fn = scrub_mod.make_exec_scrub_fn(execer, "node7", argv_prefix_fn=lambda: next(prefixes),
                                      max_mib=8)
    fn(_Gpu())
    fn(_Gpu())  # the prefix is resolved per call
    assert [c[1][:3] for c in execer.calls] == [["croagent", "scrub", "--bdf"],
                                                ["chroot", "/x", "croagent"]]
    assert execer.calls[0][1][-2:] == ["--max-mib", "8"]


def test_scrub_via_exec_error_shapes():
    # a failed scrub is reported by the agent as JSON with exit 1: passed on
    failed = {"ok": False, "rc": -40, "n_bad": 3, "msg": "residue after scrub"}
    assert scrub_mod.scrub_via_exec(_Exec(1, json.dumps(failed)), "n", _Gpu()) == failed
    assert scrub_mod.scrub_via_exec(_Exec(127, "", "croagent: not found\n"), "n", _Gpu()) == {
        "ok": False, "rc": 127, "msg": "croagent: not found"}
    assert scrub_mod.scrub_via_exec(_Exec(1, "  \n", ""), "n", _Gpu()) == {
        "ok": False, "rc": 1, "msg": "croagent scrub failed"}
    # empty output is no pass, whatever the exit status
    assert scrub_mod.scrub_via_exec(_Exec(0, "", ""), "n", _Gpu())["ok"] is False
    got = scrub_mod.scrub_via_exec(_Exec(0, "Segmentation fault", ""), "n", _Gpu())
    assert got == {"ok": False, "rc": 0, "msg": "unparseable scrub output: Segmentation fault"}
    assert scrub_mod.scrub_via_exec(_Exec(0, "[1, 2]", ""), "n", _Gpu())["ok"] is False


# -- croagent scrub without a GPU ------------------------------------------------------


@pytest.fixture(scope="module")
def agent():
    from cro_amd.hip import build as hip_build

    if not os.path.exists(AGENT):
        hip_build.build()
    if not os.path.exists(hip_build.SCRUB_OUT):
        hip_build.build_scrub()
    return AGENT


def _no_gpu():
    return not os.path.exists("/dev/kfd")


def test_croagent_scrub_without_a_gpu_reports_json_and_fails(agent):
    if not _no_gpu():
        pytest.skip("this host has a GPU; the agent's scrub on it is tests/test_scrub_gpu.py")
    for argv in (["scrub"], ["scrub", "--device", "0", "--max-mib", "64"],
                 ["scrub", "--bdf", "0000:5a:00.0", "--min-fraction", "0.5"]):
        proc = subprocess.run([agent, *argv], capture_output=True, text=True, timeout=60)
        assert proc.returncode == 1, (argv, proc.stdout, proc.stderr)
        lines = proc.stdout.strip().splitlines()
        assert len(lines) == 1, proc.stdout
        data = json.loads(lines[0])
        assert data["ok"] is False and data["rc"] == -1 and data["msg"], data


def test_croagent_without_the_scrub_library_serves_the_rest(agent, tmp_path, monkeypatch):
    """An agent built by the build's own recipe beside libcroprobe.so only:
    scrub says what is missing, every other subcommand works."""
    from cro_amd.hip import build as hip_build

    (tmp_path / "agent").mkdir()
    (tmp_path / "hip").mkdir()
    lone = tmp_path / "agent" / "croagent"
    shutil.copy(hip_build.OUT, tmp_path / "hip" / "libcroprobe.so")
    monkeypatch.setattr(hip_build, "HIP_DIR", str(tmp_path / "hip"))
    monkeypatch.setattr(hip_build, "AGENT_OUT", str(lone))
    hip_build.build_agent(force=True)
    proc = subprocess.run([str(lone), "scrub"], capture_output=True, text=True, timeout=60)
    assert proc.returncode == 1
    data = json.loads(proc.stdout)
    assert data["ok"] is False and data["rc"] == -1
    assert data["msg"].startswith("libcroscrub.so not available: ")
    proc = subprocess.run([str(lone), "pids", "--sysroot", str(tmp_path)], capture_output=True,
                          text=True, timeout=60)
    assert proc.returncode == 0 and json.loads(proc.stdout) == {"pids": []}


def test_croagent_other_subcommands_unaffected(agent, tmp_path):
    proc = subprocess.run([agent, "list", "--sysroot", str(tmp_path)], capture_output=True,
                          text=True, timeout=60)
    assert proc.returncode == 0 and json.loads(proc.stdout) == {"gpus": []}
    proc = subprocess.run([agent], capture_output=True, text=True, timeout=60)
    assert proc.returncode == 2 and "|scrub|" in proc.stderr
    assert subprocess.run([agent, "frobnicate"], capture_output=True, timeout=60).returncode == 2


# -- build ---------------------------------------------------------------------------


def test_build_scrub_inputs_and_command_line(tmp_path, monkeypatch):
    from cro_amd.hip import build as hip_build

    inputs = [hip_build.SCRUB_SRC] + hip_build.SCRUB_HEADERS
    assert {os.path.basename(p) for p in inputs} == {
        "scrub.hip", "croscrub.h", "croscrubplan.h", "crohost.h", "crointegrity.h",
        "cropattern.h"}
    assert all(os.path.exists(p) for p in inputs)
    assert os.path.basename(hip_build.SCRUB_OUT) == "libcroscrub.so"
    # every quoted include of the source, and of the headers it includes, is an input
    import re

    for path in inputs:
        with open(path) as f:
            for name in re.findall(r'#include "([^"]+)"', f.read()):
                assert os.path.join(HIP_DIR, name) in inputs, (path, name)
    # the probe library's lists do not know the new files
    assert not set(inputs[:3]) & set(hip_build.ALL_SRCS + hip_build.ALL_HEADERS)

    files = {}
    for path in inputs + [hip_build.SRC, hip_build.COVERAGE_HEADER, hip_build.AGENT_SRC]:
        name = os.path.basename(path)
        files[name] = tmp_path / name
        files[name].write_text("")
        os.utime(files[name], (100, 100))
    out = tmp_path / "libcroscrub.so"
    monkeypatch.setattr(hip_build, "SCRUB_SRC", str(files["scrub.hip"]))
    monkeypatch.setattr(hip_build, "SCRUB_HEADERS",
                        [str(files[os.path.basename(p)]) for p in hip_build.SCRUB_HEADERS])
    monkeypatch.setattr(hip_build, "SCRUB_OUT", str(out))
    commands = []

    def fake_run(argv, check):
        commands.append(argv)
        target = argv[argv.index("-o") + 1]
        open(target, "a").close()
        os.utime(target, (400, 400))

    monkeypatch.setattr(hip_build.subprocess, "run", fake_run)
    assert hip_build.build_scrub() == str(out)  # missing: built
    assert len(commands) == 1
    assert commands[0] == [hip_build.HIPCC, *hip_build.DEVICE_FLAGS, "-fPIC", "-shared",
                           str(files["scrub.hip"]), "-o", str(out)]
    assert [a for a in commands[0] if a.endswith((".hip", ".cpp"))] == [str(files["scrub.hip"])]
    commands.clear()
    hip_build.build_scrub()
    assert commands == []  # up to date
    for name in [os.path.basename(p) for p in inputs]:
        os.utime(out, (200, 200))
        os.utime(files[name], (300, 300))
        hip_build.build_scrub()
        assert len(commands) == 1, name
        commands.clear()
        os.utime(files[name], (100, 100))
    os.utime(out, (200, 200))
    for name in ("probe.hip", "crocoverage.h", "croagent.cpp"):  # not its inputs
        os.utime(files[name], (300, 300))
    hip_build.build_scrub()
    assert commands == []
    hip_build.build_scrub(force=True)
    assert len(commands) == 1
