"""GPU times of the PatchMatch refinement (csrc/patchmatch/patchmatch.hip); writes profiles/patchmatch_times.json.  Medians of
--reps windows of --inner calls between device events after a warm-up, min .. max beside (the protocol and the scene of
scripts/time_mvs.py: 512 x 512, 5 views of a textured fronto-parallel plane, 4 sources, radius 2):
  plane_cost    vggr_plane_cost of the start (the swept map's fronto-parallel planes): one cost per pixel
  step          vggr_step, one half-iteration (half the pixels, 11 candidates each), on the state as the calls leave it;
                with the bilinear samples per second that follow from the shapes if every candidate of every active pixel
                is evaluated (H W / 2 x 11 x sources x (2 r + 1)^2 per call; candidates that a whole wavefront may not
                accept are skipped, so the true number is at most this)
  refine        refine_depth from the given start, --iterations iterations: plane_init, plane_cost, 2 x iterations steps,
                outputs, with their allocations
No thresholds: the numbers are reported.  Run under its own time limit, e.g.
    timeout -k 10 300 python scripts/time_patchmatch.py
"""
import argparse
import json
import math
import os
import platform
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--planes", type=int, default=128)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patchmatch_times.json"))
    a = ap.parse_args()
    import torch
    from time_mvs import scene, windows
    from vggsfm_amd import mvs
    from vggsfm_amd import patchmatch as pm
    assert torch.cuda.is_available(), "needs an MI355X"
    frames, poses, cams = scene(a.size, seed=0)
    ref, sources, near, far = 2, [0, 1, 3, 4], 3.0, 6.0
    rays = mvs.camera_rays(cams, a.size, a.size)[0][0]
    prop = torch.cuda.get_device_properties(0)
    res = {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "memory_gb": round(prop.total_memory / 2 ** 30), "host": platform.node(), "reps": a.reps, "inner": a.inner, "size": a.size,
           "planes": a.planes, "radius": a.radius, "sources": len(sources), "iterations": a.iterations}
    spacing = (1.0 / near - 1.0 / far) / (a.planes - 1)
    start = mvs.plane_sweep(frames, poses, cams, ref, sources, near, far, a.planes, a.radius, rays=rays).depth
    dstep = pm.default_depth_step(near, far, a.planes)
    plane = pm.plane_init(start, poses, ref, rays, near, far)
    cost_fn = lambda: pm.plane_cost(frames, poses, cams, ref, sources, plane, a.radius, rays=rays)
    cost = cost_fn()
    r = {"finite_share": float(torch.isfinite(cost).double().mean()), **windows(cost_fn, a.reps, a.inner)}
    r["bilinear_samples_per_call"] = a.size * a.size * len(sources) * (2 * a.radius + 1) ** 2
    r["bilinear_samples_per_s"] = r["bilinear_samples_per_call"] / (r["ms_median"] / 1e3)
    res["plane_cost"] = r
    print("plane_cost", json.dumps(r), flush=True)
    calls = [0]

    def step_fn():
        pm.step(frames, poses, cams, ref, sources, plane, cost, near, far, 0, calls[0] & 1, dstep, radius=a.radius, rays=rays)
        calls[0] += 1
    r = windows(step_fn, a.reps, a.inner)
    r["bilinear_samples_per_call_at_most"] = a.size * a.size // 2 * 11 * len(sources) * (2 * a.radius + 1) ** 2
    r["bilinear_samples_per_s_at_most"] = r["bilinear_samples_per_call_at_most"] / (r["ms_median"] / 1e3)
    res["step"] = r
    print("step", json.dumps(r), flush=True)
    refine = lambda: pm.refine_depth(frames, poses, cams, ref, sources, near, far, start, None, a.iterations, a.radius, rays=rays,
                                     num_planes=a.planes)
    out = refine()
    valid, swept = out.depth > 0, start > 0
    err = lambda d, v: float(((1.0 / d[v].double() - 0.25).abs() / spacing).median())
    r = {"valid_share": float(valid.double().mean()), "median_error_spacings": err(out.depth, valid),
         "sweep_median_error_spacings": err(start, swept), **windows(refine, a.reps, max(1, a.inner // 4))}
    res["refine"] = r
    print("refine", json.dumps(r), flush=True)
    assert math.isfinite(res["step"]["ms_median"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
