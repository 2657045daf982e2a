#!/usr/bin/env python3
"""Flagship benchmark: MI355X composable-GPU attach→CDI-ready latency and
reconcile throughput (BASELINE.json metric) in the CONTENDED shape.

ONE operator stack — one store, one admission chain, both reconcilers with
8-way fan-out — owns ALL N GPUs on the node (rank 0).  The timed step is
BASELINE config #3: a single ComposabilityRequest composing all N GPUs in
bulk, fanned out one reconcile worker per device through the one shared
store, so store/workqueue/GIL contention is measured, not dodged (the
round-1 per-rank-operator shape measured N independent stores).  Ranks>0
only hold the torchrun barrier protocol; the operator work all contends in
one process, matching the production deployment (one operator per node).

    step = create CR(size=N) → fabric compose ×N → PCI/KFD visibility →
           CDI spec written ×N → gfx950 health probe ×N (HIP MFMA+HBM
           kernels, concurrent across workers) → Running → delete →
           drain ×N → fabric detach ×N → gone

Why not N concurrent same-model CRs: the validating webhook (reference
rule 3, composabilityrequest_webhook.go:107-128) rejects duplicate
(node, type, model) samenode requests — concurrent same-pool CRs on one
node are inadmissible BY DESIGN; the per-device fan-out happens inside
one CR.  Cross-node pool contention is measured separately (below).

A plain run sets up, warms up, times the N steps and prints the result
line.  With ``--full`` the secondary configs also run once after the timed
region and are reported as extra keys:
  single     — CR(size=1) cycles: the pure per-device overhead path
  churn      — 1→4→N→0 spec updates under the validating webhook
               (BASELINE config #4)
  contention — 4 concurrent CRs on 4 nodes drawing from ONE shared
               fabric pool of all devices (BASELINE config #5)
  async      — CM-style asynchronous fabric with a simulated compose RTT
               (CRO_BENCH_ASYNC_RTT seconds, default 2.0), so the headline
               does not rest on a zero-RTT mock

On a GPU node the device path is real (KFD sysfs enumeration, CDI JSON
writes, HIP probe per composed device); the fabric is the in-process mock
(no physical CXL fabric exists on a bench box) and PCI hot-remove is
simulated — see cro_amd/bench_harness.py.  Without a GPU the node path is
mocked (BASELINE config #1).

Output: one JSON line from rank 0.  ``value`` = p50 attach→CDI-ready
latency in ms for the size-N bulk compose (lower is better — the
reference's implicit envelope is its 30 s visibility-poll quantum through
ONE reconcile worker); ``reconciles_per_sec`` counts both
controllers in the one shared process — the GIL-contention number.
``ms_per_step`` is the wall time of one timed step (attach + detach).

So that two runs can be compared, the timed region is kept free of two
host effects that are not the operator's work.  The process confines
itself to a fixed number of neighbouring CPUs (``--cpus K``; default one
per GPU and at least 4, ``--cpus 0`` leaves the affinity alone), so the
placement of its threads is the same from run to run; and the heap built
during set-up and warm-up is frozen out of the garbage collector, so a
full collection over it cannot land in a random timed step
(``--gc-in-steps`` leaves the collector alone).  Objects the steps
allocate are still collected.  ``config.cpus`` and ``config.gc_frozen``
in the result line say what a run did.

``--dump-outputs DIR`` writes what the LAST timed step computed as
``DIR/<name>.npy`` (float64), so two builds can be compared output for
output.  Only run-to-run deterministic results are written (what the
request looked like when it reached Running, the health-probe verdicts,
what was left after teardown) — never timings or measured rates:

  request_status   [size asked, resources in status, state is Running,
                    resources Online]
  resources        one row per composed device, in inventory order:
                   [state is Online, device id present and unlike every
                    other row's, fabric CDI id present, on the target
                    node, no error]
  probe            one row per device probed in that step, same order:
                   [ok, mfma_f32_exact, rc] (no rows on the mock node path)
  probe_mfma_tile  one 16x16 tile per probed device, same order.  The step
                   keeps only the probe's exactness flag, so the probe's
                   f32 MFMA kernel is run once more after the timed steps
                   on the probe's own inputs and its product written here
  teardown         [request seen DELETED, CDI devices left on the node,
                    fabric attachments left on the node]
"""

from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys
import threading
import time


class _RecordingEvents:
    """Pass-through view of a request watch queue that remembers every
    event its consumer took — what the caller of the final timed step saw."""

    def __init__(self, inner):
        self.inner = inner
        self.seen = []

    def get(self, timeout=None):
        ev = self.inner.get(timeout=timeout)
        self.seen.append(ev)
        return ev


def _probe_inputs():
    """A(16x64) and B(64x16) exactly as the health probe builds them
    (probe.hip: one LCG stream fills A, then B, with 24-bit fractions in
    [-0.5, 0.5))."""
    import numpy as np

    K = 64
    vals = np.empty(2 * 16 * K, dtype=np.float32)
    s = 0x9E3779B9
    for i in range(vals.size):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        vals[i] = np.float32(s >> 8) / np.float32(16777216.0) - np.float32(0.5)
    return vals[: 16 * K].reshape(16, K).copy(), vals[16 * K:].reshape(K, 16).copy()


def _probe_mfma_tile(stack, device_id):
    """D(16x16) = A @ B from the health probe's f32 MFMA kernel on the
    probe's own inputs."""
    import ctypes

    import numpy as np

    from cro_amd.nodeops.probe import hip_device_for_bdf, load_library

    a, b = _probe_inputs()
    K = a.shape[1]
    d = np.zeros(256, dtype=np.float32)

    gpu = stack.ops.find_gpu(stack.node_name, device_id)
    dev = hip_device_for_bdf(gpu.pci_bdf) if gpu is not None else None
    lib = load_library(required=True)
    fptr = ctypes.POINTER(ctypes.c_float)
    lib.cro_probe_mfma_f32.argtypes = [ctypes.c_int, fptr, fptr, fptr, ctypes.c_int]
    lib.cro_probe_mfma_f32.restype = ctypes.c_int
    rc = lib.cro_probe_mfma_f32(
        dev or 0, a.ctypes.data_as(fptr), b.ctypes.data_as(fptr),
        d.ctypes.data_as(fptr), K,
    )
    if rc != 0:
        raise RuntimeError(f"f32 MFMA tile on {device_id} failed: rc={rc}")
    return d.reshape(16, 16)


def _step_outputs(stack, name, size, seen, probes) -> dict:
    """The deterministic results of one attach→detach step as float64
    arrays (layout in the module docstring)."""
    import numpy as np

    node = stack.node_name
    # real devices in enumeration order; mock ids are random per run and
    # sort after them by id
    order = {did: i for i, did in enumerate(stack.device_ids)}

    def rank(device_id):
        return (order.get(device_id, len(order)), device_id)

    running = None
    deleted = False
    for ev in seen:
        if ev.object.metadata.name != name:
            continue
        if ev.type == "DELETED":
            deleted = True
        elif ev.object.status.state == "Running":
            running = ev.object
    children = []
    if running is not None:
        children = sorted(
            running.status.resources.values(),
            key=lambda r: rank(r.device_id),
        )
    ids = [r.device_id for r in children]
    rows = [
        [
            float(r.state == "Online"),
            float(bool(r.device_id) and ids.count(r.device_id) == 1),
            float(bool(r.cdi_device_id)),
            float(r.node_name == node),
            float(not r.error),
        ]
        for r in children
    ]
    probe_rows = [
        [float(bool(pr.get("ok"))), float(bool(pr.get("mfma_f32_exact"))),
         float(pr.get("rc", 0))]
        for _, pr in sorted(probes.items(), key=lambda kv: rank(kv[0]))
    ]
    tiles = [_probe_mfma_tile(stack, did) for did in sorted(probes, key=rank)]
    if hasattr(stack.ops, "cdi"):
        cdi_left = len(stack.ops.cdi.devices(node))
    else:
        cdi_left = len(stack.ops.cdi_written.get(node, ()))
    return {
        "request_status": np.array(
            [
                float(size),
                float(len(children)),
                float(running is not None),
                float(sum(r.state == "Online" for r in children)),
            ],
            dtype=np.float64,
        ),
        "resources": np.array(rows, dtype=np.float64).reshape(len(rows), 5),
        "probe": np.array(probe_rows, dtype=np.float64).reshape(len(probe_rows), 3),
        "probe_mfma_tile": np.array(tiles, dtype=np.float64).reshape(len(tiles), 16, 16),
        "teardown": np.array(
            [float(deleted), float(cdi_left),
             float(len(stack.fabric.attached_to(node)))],
            dtype=np.float64,
        ),
    }


def _confine_to_neighbouring_cpus(k: int) -> None:
    """Restrict this process (and every thread it starts later) to the
    aligned block of ``k`` allowed CPUs around the one it runs on now.

    Where the scheduler puts the operator's threads on a large host
    differs from run to run and shows in the step time; a fixed small set
    of adjacent CPUs takes that difference away."""
    if k <= 0 or not hasattr(os, "sched_setaffinity"):
        return
    allowed = sorted(os.sched_getaffinity(0))
    if len(allowed) <= k:
        return
    here = allowed[0]
    try:
        with open("/proc/self/stat") as f:
            # field 39 (processor); the comm field may itself hold spaces
            here = int(f.read().rsplit(")", 1)[1].split()[36])
    except (OSError, ValueError, IndexError):
        pass
    pos = allowed.index(here) if here in allowed else 0
    start = min(pos - pos % k, len(allowed) - k)
    os.sched_setaffinity(0, set(allowed[start:start + k]))


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--mode", default="DRA", choices=["DRA", "DEVICE_PLUGIN"])
    p.add_argument("--no-probe", action="store_true")
    p.add_argument("--fabric-latency", type=float, default=0.0,
                   help="simulated fabric compose/decompose seconds for the "
                   "MAIN timed phase")
    p.add_argument("--fabric-async", action="store_true",
                   help="CM-style asynchronous fabric (resize+poll) for the "
                   "main phase")
    p.add_argument("--full", action="store_true",
                   help="after the timed steps also run the single/churn/"
                   "contention/async secondary configs and report them as "
                   "extra keys (a plain run measures the headline only)")
    p.add_argument("--skip-extras", action="store_true",
                   help="deprecated: a plain run no longer runs the "
                   "secondary configs; accepted so older command lines "
                   "keep working")
    p.add_argument("--dump-outputs", metavar="DIR", default="",
                   help="write what the last timed step computed as "
                   "DIR/<name>.npy (float64)")
    p.add_argument(
        "--force-detach",
        action="store_true",
        help="set force_detach on the CR spec (skips the detach load check; "
        "for test environments where another process legitimately holds a "
        "KFD context on the bench GPU)",
    )
    p.add_argument("--cpus", type=int, default=None,
                   help="confine the operator process to this many "
                   "neighbouring CPUs so runs are comparable (default: one "
                   "per GPU, at least 4; 0 = leave the CPU affinity alone)")
    p.add_argument("--gc-in-steps", action="store_true",
                   help="do not freeze the set-up heap out of the garbage "
                   "collector before the timed steps")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")

    # before torch/HIP start their threads: they inherit the mask. Only the
    # rank that runs the operator is confined.
    if int(os.environ.get("RANK", "0")) == 0:
        if args.cpus is None:
            args.cpus = max(4, args.gpus, int(os.environ.get("WORLD_SIZE", "1")))
        _confine_to_neighbouring_cpus(args.cpus)

    import torch

    dist = None
    rank, world = 0, 1
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        # NCCL needs a device per rank; with fewer, the ranks meet over gloo
        backend = (
            "nccl"
            if torch.cuda.is_available()
            and torch.cuda.device_count() >= int(os.environ["WORLD_SIZE"])
            else "gloo"
        )
        dist.init_process_group(backend=backend)
        rank = dist.get_rank()
        world = dist.get_world_size()
    local_rank = int(os.environ.get("LOCAL_RANK", rank))

    use_gpu = torch.cuda.is_available() and os.path.exists("/dev/kfd")
    if use_gpu:
        torch.cuda.set_device(local_rank % max(torch.cuda.device_count(), 1))

    n_gpus = world if world > 1 else args.gpus

    def barrier():
        if dist is not None:
            dist.barrier()
        if use_gpu:
            torch.cuda.synchronize()

    from cro_amd.bench_harness import (
        attach_detach_cycle,
        build_local_stack,
        churn_cycle,
        reconcile_count,
    )

    # Multi-rank runs: sibling ranks hold HIP/NCCL contexts on the devices
    # (torchrun protocol), which the detach load check would correctly
    # flag as foreign compute processes. force_detach (a first-class spec
    # field) skips that check for the bench job; the load check itself is
    # validated at N=1 and by tests/test_gpu.py.
    if world > 1:
        args.force_detach = True

    result = None
    if rank == 0:
        node_name = "bench-node"
        fabric_config = None
        if args.fabric_latency > 0 or args.fabric_async:
            from cro_amd.fabric.mock import MockFabricConfig

            fabric_config = MockFabricConfig(
                attach_latency=args.fabric_latency,
                detach_latency=args.fabric_latency,
                asynchronous=args.fabric_async,
            )
        stack = build_local_stack(
            node_name=node_name,
            mode=args.mode,
            use_gpu=use_gpu,
            gpu_count=n_gpus if use_gpu else None,
            mock_devices=max(8, n_gpus),
            enable_probe=use_gpu and not args.no_probe,
            fabric_config=fabric_config,
            cdi_dir=os.path.join(
                os.environ.get("TMPDIR", "/tmp"), "cro-cdi-bench"
            ),
        )
        stack.mgr.start()
        # the step size: every real device on a GPU node; n_gpus mock ones
        # on CPU (the driver's --gpus N values 1/2/4/8 → CR size 1/2/4/8)
        size = len(stack.device_ids) if use_gpu else n_gpus

        # keep the newest health-probe verdict per device (--dump-outputs)
        last_probes: dict = {}
        inner_probe = getattr(stack.ops, "probe_fn", None)
        if inner_probe is not None:

            def recording_probe(gpu):
                res = inner_probe(gpu)
                last_probes[gpu.device_id] = res
                return res

            stack.ops.probe_fn = recording_probe

        for i in range(args.warmup):  # HIP context + probe first-touch
            attach_detach_cycle(stack, f"warm-{i}", size=size,
                                force_detach=args.force_detach)

        # the final step's caller-side view of the request (--dump-outputs)
        last_events = _RecordingEvents(stack.request_events)
        last_step = args.steps - 1

        # everything allocated so far (torch, the stack, warm-up leftovers)
        # leaves the collector's sight: a full collection over that heap
        # costs 100+ ms and would land in a random timed step
        if not args.gc_in_steps:
            gc.collect()
            gc.freeze()

        barrier()
        rec0 = reconcile_count(stack)
        t_start = time.monotonic()
        samples = [
            attach_detach_cycle(stack, f"step-{i}", size=size,
                                force_detach=args.force_detach,
                                events=last_events if i == last_step else None)
            for i in range(args.steps)
        ]
        barrier()
        t_end = time.monotonic()
        rec1 = reconcile_count(stack)

        elapsed = t_end - t_start
        if args.dump_outputs:
            import numpy as np

            os.makedirs(args.dump_outputs, exist_ok=True)
            outputs = _step_outputs(
                stack, f"step-{last_step}", size, last_events.seen, last_probes
            )
            for key, arr in outputs.items():
                np.save(os.path.join(args.dump_outputs, f"{key}.npy"), arr)
        attach_ms = sorted(s["attach_ms"] for s in samples)
        detach_ms = sorted(s["detach_ms"] for s in samples)

        # attach-phase breakdown (CRO_BENCH_PHASES=<path>) — side file so
        # stdout stays the single contract JSON line
        phases_path = os.environ.get("CRO_BENCH_PHASES", "")
        if phases_path:
            phases = {}
            for metric in stack.mgr.metrics.attach_phase_seconds.collect():
                for s in metric.samples:
                    if s.name.endswith("_sum"):
                        phases.setdefault(s.labels["phase"], {})["sum_s"] = s.value
                    elif s.name.endswith("_count"):
                        phases.setdefault(s.labels["phase"], {})["count"] = s.value
            for v in phases.values():
                if v.get("count"):
                    v["avg_ms"] = round(v["sum_s"] * 1e3 / v["count"], 3)
            with open(phases_path, "w") as f:
                json.dump(phases, f, indent=2)

        extras = {}
        run_extras = args.full and not args.skip_extras
        if run_extras:
            # pure per-device overhead path (round-1 headline shape)
            singles = [
                attach_detach_cycle(stack, f"single-{i}", size=1,
                                    force_detach=args.force_detach)
                for i in range(min(args.steps, 10))
            ]
            extras["single_attach_p50_ms"] = round(
                statistics.median(s["attach_ms"] for s in singles), 3)

            # config #4: churn under the webhook
            sizes = tuple(dict.fromkeys(s for s in (1, 4, size) if s <= size))
            churn = churn_cycle(
                stack, "churn-0", sizes=sizes + (0,),
                force_detach=args.force_detach,
            )
            extras["churn_ms"] = {
                k[:-2] + "_ms": round(v * 1e3, 1) for k, v in churn.items()
            }

            # config #5: 4 concurrent CRs on 4 logical nodes drawing from
            # the ONE shared fabric pool (admission-legal cross-node
            # contention; same model, same pool, one store/operator)
            from cro_amd.api.v1alpha1.types import Node

            n_contenders = min(4, size) or 1
            per_cr = max(size // n_contenders, 1)
            cnodes = [f"{node_name}-c{j}" for j in range(n_contenders)]
            for cn in cnodes:
                nobj = Node()
                nobj.metadata.name = cn
                nobj.status.capacity.milli_cpu = 128000
                nobj.status.capacity.memory = 2 << 40
                nobj.status.capacity.allowed_pod_number = 256
                stack.mgr.client.create(nobj)
                if hasattr(stack.ops, "set_driver"):
                    stack.ops.set_driver(cn, True)

            couts = [[] for _ in range(n_contenders)]
            cerrs: list = []

            import copy as _copy

            def contender(j: int):
                # attach_detach_cycle targets stack.node_name; a shallow
                # proxy points this contender's CRs at its own node while
                # sharing the one store/manager/fabric
                proxy = _copy.copy(stack)
                proxy.node_name = cnodes[j]
                events = stack.mgr.store.watch(["ComposabilityRequest"])
                try:
                    for i in range(3):
                        couts[j].append(
                            attach_detach_cycle(
                                proxy, f"cont-{j}-{i}", size=per_cr,
                                force_detach=args.force_detach, events=events,
                            )
                        )
                except Exception as exc:
                    cerrs.append(f"contender {j}: {exc}")
                finally:
                    stack.mgr.store.stop_watch(events)

            crec0 = reconcile_count(stack)
            ct0 = time.monotonic()
            cthreads = [
                threading.Thread(target=contender, args=(j,))
                for j in range(n_contenders)
            ]
            for t in cthreads:
                t.start()
            for t in cthreads:
                t.join()
            ct1 = time.monotonic()
            if cerrs:
                raise RuntimeError("; ".join(cerrs))
            call = sorted(x["attach_ms"] for o in couts for x in o)
            extras["contention"] = {
                "n_crs": n_contenders,
                "devices_per_cr": per_cr,
                "attach_p50_ms": round(statistics.median(call), 3),
                "attach_p99_ms": round(call[max(int(len(call) * 0.99) - 1, 0)], 3),
                "reconciles_per_sec": round(
                    (reconcile_count(stack) - crec0) / (ct1 - ct0), 1),
            }
        stack.mgr.stop()

        if run_extras:
            # async-compose config: CM-style resize+poll
            # fabric with a real RTT, own small stack so the headline and
            # the async number are separate records
            from cro_amd.fabric.mock import MockFabricConfig

            rtt = float(os.environ.get("CRO_BENCH_ASYNC_RTT", "2.0"))
            astack = build_local_stack(
                node_name=node_name,
                mode=args.mode,
                use_gpu=use_gpu,
                gpu_count=1 if use_gpu else None,
                enable_probe=use_gpu and not args.no_probe,
                fabric_config=MockFabricConfig(
                    attach_latency=rtt, detach_latency=rtt, asynchronous=True,
                ),
                cdi_dir=os.path.join(
                    os.environ.get("TMPDIR", "/tmp"), "cro-cdi-bench-async"
                ),
            )
            astack.mgr.start()
            acycles = [
                attach_detach_cycle(
                    astack, f"async-{i}", size=1,
                    force_detach=args.force_detach, timeout=120.0,
                )
                for i in range(2)
            ]
            astack.mgr.stop()
            extras["async_fabric"] = {
                "rtt_s": rtt,
                "attach_p50_ms": round(
                    statistics.median(a["attach_ms"] for a in acycles), 1),
                "note": "reference first re-poll on an async fabric is ≈30 s "
                        "(composableresource_controller.go:236)",
            }

        p50 = statistics.median(attach_ms)
        result = {
            "metric": "p50 GPU attach→CDI-ready latency (ms) + reconciles/sec at 1/2/4/8 MI355X",
            "value": round(p50, 3),
            "unit": "ms",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed * 1e3 / args.steps, 3),
            "higher_is_better": False,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic",
            "reconciles_per_sec": round((rec1 - rec0) / elapsed, 1),
            "attach_p50_ms": round(p50, 3),
            "attach_p99_ms": round(attach_ms[max(int(len(attach_ms) * 0.99) - 1, 0)], 3),
            "detach_p50_ms": round(statistics.median(detach_ms), 3),
            "config": {
                "model": f"ComposabilityRequest(type=gpu, model=mi355x, size={size}) bulk compose",
                "global_batch": size,
                "seq_len": 0,
                "parallelism": (
                    f"ONE shared-store operator owning {size} device(s), "
                    f"8 reconcile workers fanning out one per device"
                ),
                "fabric": "mock (in-process; no physical CXL fabric on bench node)"
                + (f", simulated latency {args.fabric_latency}s"
                   + (" async" if args.fabric_async else "")
                   if args.fabric_latency else ""),
                "node_path": "real KFD/CDI/HIP-probe" if use_gpu else "mock",
                "device_resource_type": args.mode,
                "probe": bool(use_gpu and not args.no_probe),
                "force_detach": bool(args.force_detach),
                "cpus": (len(os.sched_getaffinity(0))
                         if hasattr(os, "sched_getaffinity") else None),
                "gc_frozen": not args.gc_in_steps,
            },
            **extras,
        }
    else:
        # non-zero ranks: hold the barrier protocol while rank 0's single
        # shared operator does the contended work
        barrier()
        barrier()

    if rank == 0 and result is not None:
        print(json.dumps(result, ensure_ascii=False))

    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
