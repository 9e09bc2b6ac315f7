"""GPU times of the reprojection video (vggsfm_amd/reproj_video.py) on a synthetic workload; writes
profiles/reproj_video_times.json.  Default size: configs[2] (200 frames x 100k points, ~5 M observations, 1024 x 1024
frames), with ``sparse_depth_device`` already computed as the runner leaves it.  Run each invocation under its own time
limit, e.g.  timeout -k 10 600 python scripts/time_reproj_video.py  (per-kernel times: under rocprofv3 --kernel-trace
--stats).

--reference-cpu N instead times the upstream CPU path (create_video_with_reprojections with OpenCV's calls stubbed out, so
without any drawing) on the first N frames of the same scene; it needs the upstream source tree (oracle.ref_harness) and
no GPU, and only serves as a host-side comparison."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vggsfm_amd import pycolmap_compat as pc  # noqa: E402
from vggsfm_amd.scene import make_scene  # noqa: E402


def scene(a):
    sc = make_scene(a.images, a.points, "SIMPLE_RADIAL", shared_camera=True, seed=0)
    rec = pc.Reconstruction.from_arrays(sc.points3D, sc.extrinsics, sc.intrinsics, sc.tracks, sc.mask,
                                        np.array([a.size, a.size]), shared_camera=True, camera_type="SIMPLE_RADIAL",
                                        extra_params=sc.extra_params)
    rec._track_csr()
    return rec


def gpu(a):
    import torch

    from vggsfm_amd import reproj_video as RV
    from vggsfm_amd.runners import GeometryConfig, GeometryRunner

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps, out

    rec = scene(a)
    runner = GeometryRunner(GeometryConfig())
    pred = runner.extract_sparse_depth_and_point_from_reconstruction({"reconstruction": rec})
    sd = pred["sparse_depth_device"]
    gen = torch.Generator(device="cuda").manual_seed(0)
    imgs = torch.randint(0, 256, (len(sd.names), a.size, a.size, 3), generator=gen, device="cuda", dtype=torch.uint8)
    images = {n: imgs[k] for k, n in enumerate(sd.names)}
    video = (a.size, a.size)
    xyz, ids = RV.live_points(rec)
    xyz_t, ids_t = torch.from_numpy(xyz).cuda(), torch.from_numpy(ids).cuda()
    res = {"images": len(sd.names), "points": int(len(xyz)), "frame": a.size, "observations": int(sd.obs_ptr[-1]),
           "draw_radius": 3}
    res["stats_ms"], _ = timed(lambda: RV.stats(xyz_t, ids_t, "dis_to_center"), a.reps)
    import matplotlib
    cmap = matplotlib.colormaps.get_cmap("gist_rainbow")
    cmap._init()
    lut = cmap._lut                                  # (resolved once, outside the timed calls)
    res["render_ms"], frames = timed(lambda: RV.render(sd, xyz_t, ids_t, images, video, cmap=lut), a.reps)
    _, dbg = RV.render(sd, xyz_t, ids_t, images, video, cmap=lut, return_debug=True)
    res["visible_observations"] = int(dbg.visible.sum())
    res["output_bytes"] = int(frames.numel())
    res["render_output_GBps"] = res["output_bytes"] / (res["render_ms"] * 1e-3) / 1e9
    res["make_reprojection_video_ms"], _ = timed(
        lambda: runner.make_reprojection_video(pred, video, [f"/x/{n}" for n in sd.names], images), max(1, a.reps // 2))
    return res


def reference_cpu(a):
    """The upstream path on the first a.reference_cpu frames (cv2 stubbed: no drawing)."""
    from oracle import ref_harness
    ref_harness.install()
    sys.modules["pycolmap"] = pc
    import warnings
    from types import SimpleNamespace
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from vggsfm.runners import runner as R
        from vggsfm.utils import utils as U

    rec = scene(a)
    pred = object.__new__(R.VGGSfMRunner).extract_sparse_depth_and_point_from_reconstruction({"reconstruction": rec})
    names = list(pred["sparse_depth"])[:a.reference_cpu]
    img = np.zeros((a.size, a.size, 3), np.uint8)
    U.cv2 = SimpleNamespace(COLOR_RGB2BGR=4, LINE_AA=16, BORDER_CONSTANT=0, cvtColor=lambda im, c: im,
                            circle=lambda *x, **k: None, copyMakeBorder=lambda im, *x, **k: im)
    t0 = time.perf_counter()
    U.create_video_with_reprojections("", (a.size, a.size), rec, names, pred["sparse_depth"], pred["sparse_point"],
                                      original_images={n: img for n in names})
    ms = (time.perf_counter() - t0) * 1e3
    obs = [len(pred["sparse_depth"][n]) for n in names]
    return {"reference_cpu_frames": len(names), "reference_cpu_ms": ms, "reference_cpu_ms_per_frame": ms / len(names),
            "reference_cpu_observations_per_frame": float(np.mean(obs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reference-cpu", type=int, default=0, metavar="N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproj_video_times.json"))
    a = ap.parse_args()
    res = reference_cpu(a) if a.reference_cpu else gpu(a)
    if os.path.exists(a.out):                      # keep the other mode's figures
        old = json.load(open(a.out))
        old.update(res)
        res = old
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
