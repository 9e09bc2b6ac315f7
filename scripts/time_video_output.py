"""GPU times of the video output tail (VideoGeometry.update_points_color / dicts_to_output, csrc/colors.hip) on the c5
world of scripts/run_c5_video.py (1000 frames; the table the loop leaves: about 250k points and 4.7 M observations),
with procedural 1024 x 1024 float32 frames (tests/video_output_frames.py) built on the device: 12.6 GB.  Writes
profiles/video_output_times.json.  Run each invocation under its own time limit, e.g.
    timeout -k 10 600 python scripts/time_video_output.py
Per-kernel times: a run of its own under  rocprofv3 --kernel-trace --stats -- python scripts/time_video_output.py --trace
(which only runs the device-frame colour step, `--reps` times; kernels color_gather_kernel / color_ptr_kernel /
color_reduce_kernel).

--host adds the host-streamed variant: the same frames in pinned host memory, streamed to the device in chunks of
--chunk frames (one pinned buffer of the whole video, so it needs 12.6 GB of host memory).

--reference-cpu P instead times the upstream ``_update_points_color`` loop on the CPU (oracle.ref_harness) on the first P
points of a table of the same shape built without the GPU: a host-side figure, for comparison only."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

from tests.video_output_frames import frames_torch  # noqa: E402
from vggsfm_amd import video as V  # noqa: E402

SEED = 17


def c5_geometry(frames):
    """The VideoGeometry that scripts/run_c5_video.py leaves after its loop (captured from VideoGeometry.run)."""
    import run_c5_video as C5
    captured = {}
    orig = V.VideoGeometry.run

    def run(self, *a, **k):
        captured["vg"] = self
        return orig(self, *a, **k)
    V.VideoGeometry.run = run
    try:
        C5.run_video(frames=frames)
    finally:
        V.VideoGeometry.run = orig
    return captured["vg"]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def gpu(a):
    vg = c5_geometry(a.frames)
    t = vg.table
    T, S = int(t.extri.shape[0]), a.size
    frames = torch.empty((T, 3, S, S), dtype=torch.float32, device="cuda")
    for f0 in range(0, T, 50):
        frames_torch(SEED, f0, min(T, f0 + 50), S, S, "cuda", out=frames[f0:min(T, f0 + 50)])
    torch.cuda.synchronize()
    res = {"frames": T, "frame": S, "points": t.num_points, "observations": t.num_observations,
           "frame_bytes": frames.numel() * 4}
    if a.trace:
        for _ in range(a.reps):
            vg.update_points_color(frames)
        torch.cuda.synchronize()
        return res
    res["update_points_color_ms"], (rgb, has) = timed(lambda: vg.update_points_color(frames), a.reps)
    res["coloured_points"] = int(has.sum())
    crop = torch.tensor([[[1920.0, 1080.0, 1, 1, 0.0, -420.0, 0, 0]]]).expand(1, T, -1)
    paths = [f"/data/c5/frame_{k:04d}.jpg" for k in range(T)]
    res["dicts_to_output_ms"], pred = timed(
        lambda: vg.dicts_to_output(0, T, paths, crop, (S, S), back_to_original_resolution=True), max(1, a.reps // 2))
    res["output_points2D"] = int(sum(len(pred["reconstruction"].images[i].points2D) for i in pred["reconstruction"].images))
    if a.host:
        host = frames.cpu().pin_memory()
        del frames
        torch.cuda.empty_cache()
        res["host_chunk_frames"] = a.chunk
        res["update_points_color_host_ms"], (rgb_h, _) = timed(lambda: vg.update_points_color(host, frame_chunk=a.chunk),
                                                               max(1, a.reps // 2))
        res["host_bit_identical"] = bool(torch.equal(rgb_h, rgb))
        res["host_stream_GBps"] = res["frame_bytes"] / (res["update_points_color_host_ms"] * 1e-3) / 1e9
    return res


def reference_cpu(a):
    """The upstream loop on a table of c5 shape built on the host (points visible over runs of consecutive frames)."""
    import types
    import warnings
    from collections import defaultdict

    import numpy as np

    from oracle import ref_harness
    ref_harness.install()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import vggsfm.runners.video_runner as VR
    rng = np.random.default_rng(0)
    T, S, P = 64, a.size, a.reference_cpu
    images = torch.from_numpy(np.zeros((1, T, 3, S, S), np.float32))
    runner = object.__new__(VR.VideoRunner)
    runner.images = images
    runner.point_dict = {}
    nobs = 0
    for p in range(P):
        n = int(rng.integers(3, 36))                                  # ~19 observations per point, as at c5
        f0 = int(rng.integers(0, T - n))
        uv = rng.uniform(0, S - 1, size=(n, 2)).astype(np.float32)
        runner.point_dict[p] = {"xyz": torch.zeros(3), "rgb": torch.zeros(3, dtype=torch.uint8),
                                "track": {f0 + k: {"uv": torch.from_numpy(uv[k]), "vis": torch.ones(1)} for k in range(n)}}
        nobs += n
    runner.frame_dict = defaultdict(dict)
    runner.cfg = types.SimpleNamespace()
    t0 = time.perf_counter()
    runner._update_points_color()
    ms = (time.perf_counter() - t0) * 1e3
    return {"reference_cpu_points": P, "reference_cpu_observations": nobs, "reference_cpu_ms": ms,
            "reference_cpu_us_per_observation": 1e3 * ms / nobs,
            "reference_cpu_note": "upstream _update_points_color on the CPU (one process), a host-side figure only"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--reference-cpu", type=int, default=0, metavar="P")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_output_times.json"))
    a = ap.parse_args()
    res = reference_cpu(a) if a.reference_cpu else gpu(a)
    if a.trace:
        print(json.dumps(res))
        return
    if os.path.exists(a.out):                      # keep the other modes' figures
        old = json.load(open(a.out))
        old.update(res)
        res = old
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
