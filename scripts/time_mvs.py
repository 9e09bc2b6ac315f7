"""GPU times of the multi-view stereo entries (csrc/mvs/mvs.hip); writes profiles/mvs_times.json.  Medians of --reps windows
of --inner calls between device events after a warm-up, min .. max beside (the method of scripts/time_klt.py):
  sweep         vggm_plane_sweep: one 512 x 512 reference view, 128 planes, 4 sources, radius 2, no cost volume; with the
                bilinear samples per second that follow from the shapes (H W planes sources (2 r + 1)^2 per call)
  filter        vggm_consistency_filter at the same size: the swept map of the reference view against maps of 4 sources
The scene: 5 cameras on a line in front of a fronto-parallel plane at depth 4 that carries a sum of Gaussian blobs on a
grid (texture everywhere), rendered by ray-plane intersection in torch; depth range 3 .. 6.  No thresholds: the numbers
are reported.  Run under its own time limit, e.g.
    timeout -k 10 300 python scripts/time_mvs.py
"""
import argparse
import json
import math
import os
import platform
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(fn, reps, inner):
    """median / min / max milliseconds per call over `reps` windows of `inner` calls between device events"""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}


def scene(size, seed):
    """frames (5,size,size) float32, poses (5,3,4), cams (5,4) float64 on the device: cameras at x = -0.4 .. 0.4 (identity
    rotation) looking at the plane z = 4, textured by one blob per 8 x 8 pixels of the middle view"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    f = 1.25 * size
    cams = torch.tensor([[f, (size - 1) / 2.0, (size - 1) / 2.0, 0.0]] * 5, dtype=torch.float64, device="cuda")
    xs = [-0.4, -0.2, 0.0, 0.2, 0.4]
    poses = torch.zeros(5, 3, 4, dtype=torch.float64, device="cuda")
    poses[:, :, :3] = torch.eye(3, dtype=torch.float64, device="cuda")
    poses[:, 0, 3] = -torch.tensor(xs, dtype=torch.float64, device="cuda")
    cells = size // 8 + 16                                    # blobs beyond the middle view's frame, for the outer cameras
    unit = 8.0 * 4.0 / f                                      # 8 px of the middle view on the plane
    cy, cx = torch.meshgrid((torch.arange(cells, device="cuda") - cells / 2 + 0.5) * unit,
                            (torch.arange(cells, device="cuda") - cells / 2 + 0.5) * unit, indexing="ij")
    cx = (cx + unit * (0.4 * torch.rand(cells, cells, generator=g, device="cuda") - 0.2)).reshape(-1, 1, 1)
    cy = (cy + unit * (0.4 * torch.rand(cells, cells, generator=g, device="cuda") - 0.2)).reshape(-1, 1, 1)
    amp = (0.3 + 0.7 * torch.rand(cells * cells, generator=g, device="cuda")).reshape(-1, 1, 1)
    sig = (unit * (0.2 + 0.2 * torch.rand(cells * cells, generator=g, device="cuda"))).reshape(-1, 1, 1)
    v, u = torch.meshgrid(torch.arange(size, device="cuda", dtype=torch.float32), torch.arange(size, device="cuda", dtype=torch.float32),
                          indexing="ij")
    frames = []
    for x0 in xs:
        px, py = (u - (size - 1) / 2.0) / f * 4.0 + x0, (v - (size - 1) / 2.0) / f * 4.0        # the plane point of each pixel
        img = torch.zeros(size, size, device="cuda")
        for c0 in range(0, cells * cells, 128):
            s = slice(c0, c0 + 128)
            img += (amp[s] * torch.exp(-((px - cx[s]) ** 2 + (py - cy[s]) ** 2) / (2 * sig[s] ** 2))).sum(0)
        frames.append(img)
    return torch.stack(frames).contiguous(), poses, cams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--planes", type=int, default=128)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvs_times.json"))
    a = ap.parse_args()
    import torch
    from vggsfm_amd import mvs
    assert torch.cuda.is_available(), "needs an MI355X"
    frames, poses, cams = scene(a.size, seed=0)
    ref, sources, near, far = 2, [0, 1, 3, 4], 3.0, 6.0
    rays, ray_index = mvs.camera_rays(cams, a.size, a.size)
    prop = torch.cuda.get_device_properties(0)
    res = {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "memory_gb": round(prop.total_memory / 2 ** 30), "host": platform.node(), "reps": a.reps, "inner": a.inner, "size": a.size,
           "planes": a.planes, "radius": a.radius, "sources": len(sources)}
    sweep = lambda v=ref, s=sources: mvs.plane_sweep(frames, poses, cams, v, s, near, far, a.planes, a.radius, rays=rays[0])
    out = sweep()
    valid = out.index >= 0
    err = (1.0 / out.depth[valid].double() - 0.25).abs() / ((1.0 / near - 1.0 / far) / (a.planes - 1))
    r = {"valid_share": float(valid.double().mean()), "median_error_spacings": float(err.median()), **windows(sweep, a.reps, a.inner)}
    r["bilinear_samples_per_call"] = a.size * a.size * a.planes * len(sources) * (2 * a.radius + 1) ** 2
    r["bilinear_samples_per_s"] = r["bilinear_samples_per_call"] / (r["ms_median"] / 1e3)
    res["sweep"] = r
    print("sweep", json.dumps(r), flush=True)
    depth = torch.stack([sweep(v, [s for s in range(5) if s != v][:4]).depth for v in range(5)])
    flt = lambda: mvs.filter_consistent(depth, poses, cams, ref, sources, rays=rays, ray_index=ray_index)
    kept = flt().depth > 0
    r = {"kept_share": float(kept.double().mean()), **windows(flt, a.reps, 10 * a.inner)}
    r["pixels_per_s"] = a.size * a.size / (r["ms_median"] / 1e3)
    res["filter"] = r
    print("filter", json.dumps(r), flush=True)
    assert math.isfinite(res["sweep"]["ms_median"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
