"""GPU-marked tests: run on a real MI355X (gpurun / driver round-end).

Covers: KFD enumeration of real hardware, the gfx950 HIP health probe
(including MFMA numerics against a PyTorch fp32 reference), and the full
attach→CDI-ready→detach lifecycle on the real node path.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _require_gpu():
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU (KFD) on this host")


def test_kfd_enumeration_real():
    _require_gpu()
    from cro_amd.nodeops.execs import LocalNodeExec
    from cro_amd.nodeops.kfd import enumerate_gpus

    gpus = enumerate_gpus(LocalNodeExec(), "local")
    assert len(gpus) >= 1
    g = gpus[0]
    assert g.device_id.startswith("GPU-")
    assert g.render_minor >= 128
    assert os.path.exists(g.render_path), g.render_path
    # MI355X: 288 GB HBM3E per GPU
    assert g.vram_bytes > 250 * (1 << 30), f"vram {g.vram_bytes}"


def test_probe_extension_loads_and_passes():
    _require_gpu()
    from cro_amd.nodeops.probe import run_probe

    result = run_probe(0)
    assert result["ok"], result
    assert result["mfma_f32_exact"], "matrix pipe produced wrong f32 results"
    assert "gfx950" in result["gcn_arch"], result["gcn_arch"]
    # healthy MI355X floors (loose: probe gates, not peak tuning)
    assert result["hbm_gbps"] > 2000, result
    assert result["bf16_tflops"] > 500, result
    assert result["vram_total"] > 250 * (1 << 30)


def test_mfma_f32_numerics_vs_torch():
    """GPU MFMA tile vs plain PyTorch fp32 reference of the same op."""
    _require_gpu()
    import ctypes

    import torch

    from cro_amd.nodeops.probe import load_library

    lib = load_library(required=True)
    lib.cro_probe_mfma_f32.argtypes = [
        ctypes.c_int,
        ctypes.POINTER(ctypes.c_float),
        ctypes.POINTER(ctypes.c_float),
        ctypes.POINTER(ctypes.c_float),
        ctypes.c_int,
    ]
    K = 128
    rng = np.random.default_rng(7)
    A = rng.standard_normal((16, K), dtype=np.float32)
    B = rng.standard_normal((K, 16), dtype=np.float32)
    D = np.zeros((16, 16), dtype=np.float32)
    rc = lib.cro_probe_mfma_f32(
        0,
        A.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
        B.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
        D.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
        K,
    )
    assert rc == 0
    ref = (torch.from_numpy(A) @ torch.from_numpy(B)).numpy()
    np.testing.assert_allclose(D, ref, rtol=2e-6, atol=1e-5)
    # and exactly: the k-ordered fmaf chain, bit for bit (more shapes and the
    # edge cases in tests/test_probe_quick_gpu.py)
    from cro_amd.nodeops.probe import fmaf_chain

    chain, ties = fmaf_chain(A, B)
    assert ties == 0  # the numpy chain is the true one for this input
    assert np.array_equal(D.view(np.uint32), chain.view(np.uint32))


def test_full_lifecycle_real_node_path():
    """Attach→CDI-ready→detach on the real device path (config #2)."""
    _require_gpu()
    from cro_amd.bench_harness import attach_detach_cycle, build_local_stack

    cdi_dir = os.path.join(os.environ.get("TMPDIR", "/tmp"), "cro-cdi-gputest")
    stack = build_local_stack(node_name="gputest", use_gpu=True, gpu_index=0, cdi_dir=cdi_dir)
    stack.mgr.start()
    try:
        timing = attach_detach_cycle(stack, "gpu-e2e", size=1, timeout=180)
        # must beat the reference's 30 s visibility-poll quantum outright
        assert timing["attach_ms"] < 30000, timing
        # CDI spec cleaned up after detach
        assert stack.ops.cdi.devices("gputest") == []
    finally:
        stack.mgr.stop()


def test_cdi_spec_contents_on_real_gpu():
    _require_gpu()
    from cro_amd.nodeops.amdgpu import AmdNodeOps
    from cro_amd.nodeops.execs import LocalNodeExec
    from cro_amd.nodeops.kfd import enumerate_gpus

    ex = LocalNodeExec()
    gpus = enumerate_gpus(ex, "local")
    cdi_dir = os.path.join(os.environ.get("TMPDIR", "/tmp"), "cro-cdi-spec-test")
    ops = AmdNodeOps(ex, cdi_dir=cdi_dir, destructive=False)
    cdi_id = ops.write_cdi("local", gpus[0].device_id)
    assert cdi_id == f"amd.com/gpu={gpus[0].device_id}"
    spec_file = os.path.join(cdi_dir, "amd.com-gpu-cro.json")
    with open(spec_file) as f:
        spec = json.load(f)
    dev = spec["devices"][0]
    for node in dev["containerEdits"]["deviceNodes"]:
        assert os.path.exists(node["path"]), node["path"]
    ops.remove_cdi("local", gpus[0].device_id)


def test_bench_one_gpu_quick():
    _require_gpu()
    proc = subprocess.run(
        # --force-detach: this pytest process already holds a KFD context
        # on the bench GPU (probe tests above), which the subprocess's
        # detach load-check would legitimately see as foreign load
        [sys.executable, "bench.py", "--steps", "5", "--warmup", "2", "--force-detach"],
        cwd=REPO,
        capture_output=True,
        text=True,
        timeout=600,
    )
    assert proc.returncode == 0, f"stdout:\n{proc.stdout}\nstderr:\n{proc.stderr}"
    result = json.loads(proc.stdout.strip().splitlines()[-1])
    assert result["config"]["node_path"] == "real KFD/CDI/HIP-probe"
    assert result["value"] < 30000  # ms; beat the reference's poll quantum


def test_split_deployment_real_node_path():
    """Cluster topology on real hardware: uvicorn API server (store +
    admission), operator over RemoteClient watch streams, REAL amdgpu node
    path (KFD/CDI/probe)."""
    _require_gpu()
    import socket
    import threading
    import time

    import httpx
    import uvicorn

    from cro_amd.api.v1alpha1.types import ComposabilityRequest, Node
    from cro_amd.controllers import build_manager
    from cro_amd.fabric.adapter import Adapter
    from cro_amd.fabric.mock import MockFabric
    from cro_amd.nodeops.amdgpu import AmdNodeOps
    from cro_amd.nodeops.execs import LocalNodeExec
    from cro_amd.nodeops.kfd import enumerate_gpus
    from cro_amd.runtime.remote import RemoteClient
    from cro_amd.server.api import build_app
    from tests.conftest import make_request

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()

    server_mgr = build_manager(Adapter("DRA", MockFabric()), None)
    server = uvicorn.Server(
        uvicorn.Config(build_app(server_mgr.client), host="127.0.0.1", port=port,
                       log_level="error")
    )
    thread = threading.Thread(target=server.run, daemon=True)
    thread.start()
    deadline = time.monotonic() + 15
    while time.monotonic() < deadline:
        try:
            if httpx.get(f"http://127.0.0.1:{port}/healthz", timeout=1).status_code == 200:
                break
        except Exception:
            time.sleep(0.05)

    execer = LocalNodeExec()
    gpus = enumerate_gpus(execer, "gpunode")[:1]
    fabric = MockFabric(bind_inventory=[
        {"device_id": g.device_id, "cdi_device_id": f"amd.com/gpu={g.device_id}",
         "model": "mi355x"} for g in gpus
    ])
    remote = RemoteClient(f"http://127.0.0.1:{port}")
    mgr = build_manager(Adapter("DRA", fabric), None, client=remote, enable_webhook=False)
    cdi_dir = os.path.join(os.environ.get("TMPDIR", "/tmp"), "cro-cdi-split")
    ops = AmdNodeOps(
        execer, client=mgr.client, cdi_dir=cdi_dir, destructive=False,
        initially_detached=[g.device_id for g in gpus],
    )
    mgr.resource_reconciler.node_ops = ops
    orig_add = fabric.add_resource

    def add_resource(resource):
        did, cdi = orig_add(resource)
        ops.simulate_compose(resource.spec.target_node, did)
        return did, cdi

    fabric.add_resource = add_resource
    node = Node()
    node.metadata.name = "gpunode"
    remote.create(node)
    mgr.start()
    try:
        remote.create(make_request("split-r1", size=1, target_node="gpunode"))
        deadline = time.monotonic() + 60
        while time.monotonic() < deadline:
            req = remote.try_get(ComposabilityRequest, "split-r1")
            if req is not None and req.status.state == "Running":
                break
            time.sleep(0.05)
        req = remote.get(ComposabilityRequest, "split-r1")
        assert req.status.state == "Running", req.status
        device_id = next(iter(req.status.resources.values())).device_id
        assert device_id == gpus[0].device_id  # the real GPU, over HTTP
        assert ops.cdi.devices("gpunode") == [device_id]

        remote.delete(ComposabilityRequest, "split-r1")
        deadline = time.monotonic() + 60
        while time.monotonic() < deadline:
            if remote.try_get(ComposabilityRequest, "split-r1") is None:
                break
            time.sleep(0.05)
        assert remote.try_get(ComposabilityRequest, "split-r1") is None
        assert ops.cdi.devices("gpunode") == []
    finally:
        mgr.stop()
        remote.close()
        server.should_exit = True
        thread.join(timeout=5)


def test_churn_races_on_real_node_path():
    """Abort-mid-attach races against the REAL node path: requests deleted
    at random points of their lifecycle must never leak CDI entries or
    fabric attachments (the syncer heals the crash-window leaks)."""
    _require_gpu()
    import random
    import time

    from cro_amd.api.v1alpha1.types import ComposabilityRequest
    from cro_amd.bench_harness import build_local_stack
    from tests.conftest import make_request

    stack = build_local_stack(
        node_name="gpuchurn", use_gpu=True, gpu_index=0,
        cdi_dir=os.path.join(os.environ.get("TMPDIR", "/tmp"), "cro-cdi-churn"),
        syncer_period=0.5, syncer_grace=2.0,
    )
    stack.mgr.start()
    rng = random.Random(7)
    try:
        for i in range(25):
            name = f"churn-{i}"
            req = make_request(name, size=1, target_node="gpuchurn")
            stack.mgr.client.create(req)
            time.sleep(rng.random() * 0.02)  # abort at a random point
            stack.mgr.client.delete(ComposabilityRequest, name)
            assert stack.mgr.wait_for(
                lambda: stack.mgr.client.try_get(ComposabilityRequest, name) is None,
                timeout=30,
            ), f"cycle {i} wedged"
        # converged: nothing attached, CDI clean (allow the syncer a moment
        # for any crash-window leak)
        assert stack.mgr.wait_for(
            lambda: stack.fabric.attached_to("gpuchurn") == [], timeout=20
        )
        assert stack.ops.cdi.devices("gpuchurn") == []
    finally:
        stack.mgr.stop()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_full_lifecycle_device_plugin_mode():
    """The DEVICE_PLUGIN half of the hardware matrix: same real node path
    (KFD, CDI, probe) with node-wide load checks and plugin-daemonset
    refresh semantics instead of DRA ResourceSlices/taints."""
    _require_gpu()
    from cro_amd.api.v1alpha1.types import DeviceTaintRule, ResourceSlice
    from cro_amd.bench_harness import attach_detach_cycle, build_local_stack

    cdi_dir = os.path.join(os.environ.get("TMPDIR", "/tmp"), "cro-cdi-gputest-dp")
    stack = build_local_stack(
        node_name="gputest-dp", use_gpu=True, gpu_index=0,
        cdi_dir=cdi_dir, mode="DEVICE_PLUGIN",
    )
    stack.mgr.start()
    try:
        timing = attach_detach_cycle(
            stack, "gpu-e2e-dp", size=1, timeout=180, force_detach=True,
        )
        assert timing["attach_ms"] < 30000, timing
        assert stack.ops.cdi.devices("gputest-dp") == []
        # DEVICE_PLUGIN mode must not have used the DRA reflection kinds
        assert stack.mgr.client.list(DeviceTaintRule) == []
    finally:
        stack.mgr.stop()
