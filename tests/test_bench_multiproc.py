"""Multi-process distributed bench path: world_size=2 over gloo on CPU —
validates the torchrun contract (rank gathering, rank-0 JSON line) that the
driver uses for the N-GPU scaling bench."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_bench_two_ranks_gloo():
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    # the CPU/gloo contract is what this test is about: hide any GPU from
    # the ranks, or a GPU node picks NCCL and two ranks cannot share the
    # one device it may have
    env["HIP_VISIBLE_DEVICES"] = "-1"
    env["CUDA_VISIBLE_DEVICES"] = "-1"
    proc = subprocess.run(
        [
            sys.executable,
            "-m",
            "torch.distributed.run",
            "--nnodes=1",
            "--nproc-per-node=2",
            "--master-addr=127.0.0.1",
            "--master-port=29517",
            "bench.py",
            "--gpus",
            "2",
            "--steps",
            "4",
            "--warmup",
            "1",
            "--full",
        ],
        cwd=REPO,
        env=env,
        capture_output=True,
        text=True,
        timeout=280,
    )
    assert proc.returncode == 0, f"stdout:\n{proc.stdout}\nstderr:\n{proc.stderr}"
    json_lines = [
        line for line in proc.stdout.splitlines() if line.startswith('{"metric"')
    ]
    assert len(json_lines) == 1, proc.stdout
    result = json.loads(json_lines[0])
    assert result["n_gpus"] == 2
    assert result["steps"] == 4
    assert result["value"] > 0
    assert result["higher_is_better"] is False
    assert result["scaling"] == "weak"
    assert result["reconciles_per_sec"] > 0
    # ONE shared-store operator on rank 0 (contended shape)
    assert result["config"]["parallelism"].startswith("ONE shared-store operator")
    assert result["config"]["global_batch"] == 2  # CR size = N
    # secondary configs ride along (configs #4/#5 + async compose)
    assert "churn_ms" in result
    assert result["contention"]["n_crs"] >= 2
    assert result["async_fabric"]["attach_p50_ms"] > 1000


def test_bench_single_process_no_dist():
    proc = subprocess.run(
        [sys.executable, "bench.py", "--steps", "3", "--warmup", "1",
         "--skip-extras"],
        cwd=REPO,
        capture_output=True,
        text=True,
        timeout=120,
    )
    assert proc.returncode == 0, proc.stderr
    result = json.loads(proc.stdout.strip().splitlines()[-1])
    assert result["n_gpus"] == 1
    assert result["value"] > 0


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run reports the headline only (secondary configs need
    --full) and --dump-outputs writes the last timed step's results."""
    import numpy as np

    out_dir = tmp_path / "outputs"
    proc = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "2", "--steps", "3",
         "--warmup", "1", "--force-detach", "--dump-outputs", str(out_dir)],
        cwd=REPO,
        capture_output=True,
        text=True,
        timeout=120,
    )
    assert proc.returncode == 0, proc.stderr
    result = json.loads(proc.stdout.strip().splitlines()[-1])
    assert result["steps"] == 3
    assert result["ms_per_step"] > 0
    assert result["unit"] == "ms" and result["higher_is_better"] is False
    for key in ("single_attach_p50_ms", "churn_ms", "contention", "async_fabric"):
        assert key not in result, key

    arrays = {f.stem: np.load(f) for f in out_dir.glob("*.npy")}
    assert set(arrays) == {
        "request_status", "resources", "probe", "probe_mfma_tile", "teardown",
    }
    assert all(a.dtype == np.float64 for a in arrays.values())
    # every device asked for is in the Running status and Online (2 mock
    # devices without a GPU; on a GPU node as many real ones, up to 2)
    size = result["config"]["global_batch"]
    assert 1 <= size <= 2
    assert arrays["request_status"].tolist() == [size, size, 1.0, size]
    assert arrays["resources"].tolist() == [[1.0] * 5] * size
    # one passing HIP probe verdict per device on the real node path, none
    # on the mock one
    probed = size if result["config"]["probe"] else 0
    assert arrays["probe"].tolist() == [[1.0, 1.0, 0.0]] * probed
    assert arrays["probe"].shape == (probed, 3)
    # the probe's f32 MFMA product per probed device against a float64
    # matmul of the same inputs: 64 products below 0.25 each, so float32
    # accumulation stays within 64 * 2^-24 * 16 < 1e-4 of it
    import bench

    a, b = bench._probe_inputs()
    ref = a.astype(np.float64) @ b.astype(np.float64)
    assert arrays["probe_mfma_tile"].shape == (probed, 16, 16)
    for tile in arrays["probe_mfma_tile"]:
        np.testing.assert_allclose(tile, ref, rtol=0, atol=1e-4)
    # request gone, no CDI entry and no fabric attachment left behind
    assert arrays["teardown"].tolist() == [1.0, 0.0, 0.0]


def test_bench_steadying_is_recorded_and_can_be_turned_off():
    """By default the run confines itself to a few CPUs and freezes the
    set-up heap out of the collector; both are reported in the result line
    and both can be switched off."""
    allowed = len(os.sched_getaffinity(0))

    def run(*extra):
        proc = subprocess.run(
            [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
             "--force-detach", *extra],
            cwd=REPO,
            capture_output=True,
            text=True,
            timeout=120,
        )
        assert proc.returncode == 0, proc.stderr
        return json.loads(proc.stdout.strip().splitlines()[-1])["config"]

    config = run()
    assert config["cpus"] == min(4, allowed)
    assert config["gc_frozen"] is True
    config = run("--cpus", "0", "--gc-in-steps")
    assert config["cpus"] == allowed
    assert config["gc_frozen"] is False
