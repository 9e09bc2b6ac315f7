"""The plain benchmark command line, `bench.py --gpus 1 --steps K --warmup W`: the timed steps and the line, nothing else.

Its headline keys mean what they do in a `--full` run; every leg that only `--full` runs (the HIP-event pass with its
per-kernel times and roofline, the scaling legs, the CPU baseline and the GPU-vs-port comparisons, triangulation, pipeline,
the configs[4] video) is null, and --dump-outputs still writes the state after the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_is_the_headline_alone(tmp_path):
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == "BA LM-iterations/sec" and out["unit"] == "LM-iterations/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 1
    assert out["value"] > 0 and abs(out["value"] - 1e3 / out["ms_per_step"]) <= 1e-6 * out["value"]
    cfg = out["config"]
    assert cfg["frames"] == 200 and cfg["tracks_per_gpu"] == 100000 and cfg["reduced_system"] == 1202
    assert cfg["kernel_ms"] is None and out["ms_per_step_with_events"] is None
    for key in ("roofline", "roofline_by_kernel", "cpu_baseline", "pose_delta_vs_port", "pose_delta_vs_port_c3",
                "pose_delta_vs_port_c4", "pose_delta_vs_port_c5_joint", "video_c5", "strong_scaling_c4",
                "strong_scaling_c4_speedup_vs_n1", "n1_same_problem", "weak_scaling_c3", "triangulation", "pipeline"):
        assert out[key] is None, key
    # the iteration's algorithmic roofline needs no run of its own
    assert out["iteration_roofline"]["algorithmic_flops"] > 0
    names = sorted(os.listdir(dump))
    assert {"cost.npy", "extrinsics.npy", "intrinsics.npy", "extra_params.npy"} <= set(names), names
    assert any(n.startswith("points3D") for n in names), names
    cost = np.load(dump / "cost.npy")
    assert cost.shape == (2,) and 0 < cost[1] <= cost[0]
