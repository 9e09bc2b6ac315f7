"""GPU times of the depth-map fusion entries (csrc/fuse/fuse.hip); writes profiles/fusion_times.json.  Medians of --reps
windows of --inner calls between device events after a warm-up, min .. max beside (the method of scripts/time_mvs.py):
  normals       vggf_depth_normals: all views of 512 x 512 in one launch
  fuse_view     vggf_fuse_view: one view against 4 sources (both launches), outputs pre-allocated, no host read
  fuse          fusion.fuse_depth_maps: every view in turn with its allocations and its two host reads, the normal map given
at 5 and at 9 views.  The scene: cameras on a line in front of a fronto-parallel plane at depth 4; the depth maps are the
plane's true depth rounded to float32, so every pixel has depth and every source confirms what it sees.  No thresholds: the
numbers are reported; the parent commit has nothing to compare with.  Run under its own time limit, e.g.
    timeout -k 10 300 python scripts/time_fusion.py
"""
import argparse
import json
import math
import os
import platform
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_mvs import windows  # noqa: E402


def scene(size, views):
    """depth (V,size,size) float32, colours (V,3,size,size) float32, poses (V,3,4), cams (V,4) on the device: cameras at
    x = -0.4 .. 0.4 (identity rotation) in front of the plane z = 4"""
    import torch
    f = 1.25 * size
    cams = torch.tensor([[f, (size - 1) / 2.0, (size - 1) / 2.0, 0.0]] * views, dtype=torch.float64, device="cuda")
    poses = torch.zeros(views, 3, 4, dtype=torch.float64, device="cuda")
    poses[:, :, :3] = torch.eye(3, dtype=torch.float64, device="cuda")
    poses[:, 0, 3] = -torch.linspace(-0.4, 0.4, views, dtype=torch.float64, device="cuda")
    depth = torch.full((views, size, size), 4.0, dtype=torch.float32, device="cuda")
    colors = torch.rand(views, 3, size, size, generator=torch.Generator(device="cuda").manual_seed(0), device="cuda")
    return depth, colors, poses, cams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_times.json"))
    a = ap.parse_args()
    import torch
    from vggsfm_amd import _lib_fuse as F
    from vggsfm_amd import fusion, mvs
    assert torch.cuda.is_available(), "needs an MI355X"
    prop = torch.cuda.get_device_properties(0)
    res = {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "memory_gb": round(prop.total_memory / 2 ** 30), "host": platform.node(), "reps": a.reps, "inner": a.inner, "size": a.size}
    L = F.lib()
    for views in (5, 9):
        depth, colors, poses, cams = scene(a.size, views)
        rays, ray_index = mvs.camera_rays(cams, a.size, a.size)
        sources = [sorted(range(views), key=lambda s: (abs(s - v), s))[1:5] for v in range(views)]
        normals = fusion.depth_normals(depth, poses, cams, rays=rays, ray_index=ray_index)
        r = {"normals": windows(lambda: fusion.depth_normals(depth, poses, cams, rays=rays, ray_index=ray_index), a.reps, a.inner)}
        r["normals"]["pixels_per_s"] = views * a.size * a.size / (r["normals"]["ms_median"] / 1e3)
        # one view through the entry itself, everything allocated before the window
        plane = a.size * a.size
        dev = depth.device
        claimed = torch.zeros(views, a.size, a.size, dtype=torch.uint8, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        out = [torch.empty(plane, 3, dtype=torch.float64, device=dev), torch.empty(plane, 3, dtype=torch.float32, device=dev),
               torch.empty(plane, 3, dtype=torch.float32, device=dev)] + [torch.empty(plane, dtype=torch.int32, device=dev) for _ in range(3)]
        stage = [torch.empty(plane, dtype=torch.int32, device=dev), torch.empty(plane, 3, dtype=torch.float64, device=dev),
                 torch.empty(plane, 3, dtype=torch.float32, device=dev), torch.empty(plane, 3, dtype=torch.float32, device=dev),
                 torch.empty(-(-plane // F.BLOCK), dtype=torch.int32, device=dev)]
        mid = views // 2
        src = torch.tensor(sources[mid], dtype=torch.int32)

        def one_view():
            F.check(L.vggf_fuse_view(depth, normals, colors, poses, cams, rays, ray_index, rays.shape[0], views, a.size, a.size, mid,
                                     src, src.numel(), 0.01, 1.0, math.cos(math.radians(30.0)), 2, claimed, *stage, counts[0:],
                                     counts[1:], plane, *out, F.stream_ptr()), "vggf_fuse_view")
        r["fuse_view"] = windows(one_view, a.reps, a.inner)
        r["fuse_view"]["points"] = int(counts[1])
        r["fuse_view"]["pixels_per_s"] = plane / (r["fuse_view"]["ms_median"] / 1e3)
        whole = lambda: fusion.fuse_depth_maps(depth, poses, cams, sources, colors, normals, rays=rays, ray_index=ray_index)
        cloud = whole()
        r["fuse"] = windows(whole, a.reps, max(1, a.inner // 4))
        r["fuse"]["points"] = int(len(cloud.xyz))
        r["fuse"]["pixels_with_depth"] = int((depth > 0).sum())
        r["fuse"]["pixels_per_s"] = views * plane / (r["fuse"]["ms_median"] / 1e3)
        res[f"views_{views}"] = r
        print(f"views_{views}", json.dumps(r), flush=True)
        assert math.isfinite(r["fuse"]["ms_median"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
