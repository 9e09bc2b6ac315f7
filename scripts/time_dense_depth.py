"""Per-stage GPU times of the dense depth stage (vggsfm_amd/dense_depth.py) on a synthetic workload; writes
profiles/dense_depth_times.json.  Default size: configs[2] (200 images x 100k points, 1024 x 1024 maps).  Run each
invocation under its own time limit, e.g.  timeout -k 10 600 python scripts/time_dense_depth.py"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vggsfm_amd import dense_depth as DD  # noqa: E402
from vggsfm_amd import pycolmap_compat as pc  # noqa: E402
from vggsfm_amd.scene import make_scene  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_depth_times.json"))
    a = ap.parse_args()
    sc = make_scene(a.images, a.points, "SIMPLE_RADIAL", shared_camera=True, seed=0)
    rec = pc.Reconstruction.from_arrays(sc.points3D, sc.extrinsics, sc.intrinsics, sc.tracks, sc.mask,
                                        np.array([1024, 1024]), shared_camera=True, camera_type="SIMPLE_RADIAL",
                                        extra_params=sc.extra_params)
    rec._track_csr()
    res = {"images": a.images, "points": a.points, "map": a.size}
    res["sparse_ms"], sd = timed(lambda: DD.sparse_depth(rec), a.reps)
    res["observations"] = int(sd.obs_ptr[-1])
    S = len(sd.names)
    gen = torch.Generator(device="cuda").manual_seed(0)
    maps = torch.rand((S, a.size, a.size), generator=gen, device="cuda", dtype=torch.float32) * 0.3 + 0.1
    packed0 = DD.pack_maps(list(maps))
    res["align_ms"], al = timed(lambda: DD.align(packed0, sd.uvd, sd.obs_ptr, seed=1), a.reps)
    res["align_trials_max"] = int(al.n_trials.max())
    res["align_status_ok"] = bool((al.status == 0).all())
    work = packed0.flat.clone()
    packed = DD.Packed(work, packed0.off, packed0.heights, packed0.widths, packed0.max_pixels)

    def apply():
        work.copy_(packed0.flat)
        return DD.apply(packed, al.scale, al.shift)
    res["apply_plus_copy_ms"], depth = timed(apply, a.reps)
    res["copy_only_ms"], _ = timed(lambda: work.copy_(packed0.flat), a.reps)
    res["apply_ms"] = res["apply_plus_copy_ms"] - res["copy_only_ms"]
    px = S * a.size * a.size
    res["apply_bytes"] = px * 12          # read disp, write disp, write depth (float32)
    res["apply_GBps"] = res["apply_bytes"] / (res["apply_ms"] * 1e-3) / 1e9
    ids = {rec.images[i].name: i for i in rec.images}
    _, cam = DD._camera_rows(rec, [ids[n] for n in sd.names])
    inv = [rec.images[ids[n]].cam_from_world.inverse() for n in sd.names]
    inv_pose = np.stack([np.concatenate([t.rotation.matrix(), t.translation[:, None]], axis=1) for t in inv])
    res["unproject_ms"], (xyz, _) = timed(lambda: DD.unproject(packed, depth, cam, inv_pose), a.reps)
    res["valid_pixels"] = int(xyz.shape[0])
    res["unproject_with_host_copy_ms"], _ = timed(lambda: DD.unproject(packed, depth, cam, inv_pose)[0].cpu(), max(1, a.reps // 2))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
