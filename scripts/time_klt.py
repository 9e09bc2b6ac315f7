"""GPU times of the tracker's entries (csrc/klt/klt.hip); writes profiles/klt_times.json.  Medians of --reps windows of
--inner calls between device events after a warm-up, min .. max beside:
  pyramid       vggk_pyramid: 8 frames of 512 x 512 x 3, 3 levels
  detector      vggk_corner_response + vggk_local_maxima + the torch selection, one 512 x 512 frame, 2048 corners asked
  lk            vggk_lk_track, one step at 1 k and 20 k tracks, r = 7, 3 levels, epsilon = 0.01, at most 30 iterations per
                level, the second frame shifted by (3.2, -2.1) px; with the mean iteration count and the window samples per
                second that follow from it ((2 r + 1)^2 bilinear samples per track and iteration)
The frames are sums of Gaussian blobs on a grid (texture everywhere).  No thresholds: the numbers are reported.  Run under
its own time limit, e.g.
    timeout -k 10 300 python scripts/time_klt.py
"""
import argparse
import json
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


def frames(n, size, shift, seed):
    """n frames (n,3,size,size) of one blob texture, frame f translated by f x shift"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    cells = size // 8
    cy, cx = torch.meshgrid(torch.arange(cells, device="cuda") * 8.0 + 4, torch.arange(cells, device="cuda") * 8.0 + 4, indexing="ij")
    cx = (cx + 3 * torch.rand(cells, cells, generator=g, device="cuda") - 1.5).reshape(-1, 1, 1)
    cy = (cy + 3 * torch.rand(cells, cells, generator=g, device="cuda") - 1.5).reshape(-1, 1, 1)
    amp = (0.3 + 0.7 * torch.rand(cells * cells, generator=g, device="cuda")).reshape(-1, 1, 1)
    sig = (1.5 + 1.5 * torch.rand(cells * cells, generator=g, device="cuda")).reshape(-1, 1, 1)
    y, x = torch.meshgrid(torch.arange(size, device="cuda", dtype=torch.float32), torch.arange(size, device="cuda", dtype=torch.float32),
                          indexing="ij")
    out = []
    for f in range(n):
        img = torch.zeros(size, size, device="cuda")
        for c0 in range(0, cells * cells, 256):
            s = slice(c0, c0 + 256)
            img += (amp[s] * torch.exp(-((x - cx[s] - f * shift[0]) ** 2 + (y - cy[s] - f * shift[1]) ** 2) / (2 * sig[s] ** 2))).sum(0)
        out.append(img)
    return torch.stack(out)[:, None].expand(n, 3, size, size).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--tracks", default="1000,20000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "klt_times.json"))
    a = ap.parse_args()
    import torch
    from vggsfm_amd import klt
    assert torch.cuda.is_available(), "needs an MI355X"
    shift, radius, levels = (3.2, -2.1), 7, 3
    fr = frames(8, a.size, shift, seed=0)
    prop = torch.cuda.get_device_properties(0)
    res = {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "memory_gb": round(prop.total_memory / 2 ** 30), "host": platform.node(), "reps": a.reps, "inner": a.inner, "size": a.size, "levels": levels,
           "radius": radius}
    res["pyramid"] = {"frames": 8, **windows(lambda: klt.build_pyramid(fr, levels), a.reps, a.inner)}
    print("pyramid", json.dumps(res["pyramid"]), flush=True)
    pyr = klt.build_pyramid(fr, levels)
    corners = klt.detect_features(pyr, 0, 2048)
    res["detector"] = {"corners": int(corners.shape[0]), **windows(lambda: klt.detect_features(pyr, 0, 2048), a.reps, a.inner),
                       "response_only": windows(lambda: klt.corner_response(pyr, 0, 2), a.reps, a.inner)}
    print("detector", json.dumps(res["detector"]), flush=True)
    res["lk"] = {}
    g = torch.Generator(device="cuda").manual_seed(1)
    for n in (int(v) for v in a.tracks.split(",")):
        pts = (16 + (a.size - 32) * torch.rand(n, 2, generator=g, device="cuda", dtype=torch.float64)).contiguous()
        pos, status, zncc, iters = klt.track_pair(pyr, 0, 1, pts, radius=radius)
        ok = status == klt.OK
        err = (pos - pts - torch.tensor(shift, device="cuda", dtype=torch.float64)).norm(dim=1)[ok]
        r = {"tracks": n, "ok": int(ok.sum()), "mean_iterations": float(iters.double().mean()),
             "median_error_px": float(err.median()), **windows(lambda: klt.track_pair(pyr, 0, 1, pts, radius=radius), a.reps, a.inner)}
        r["window_samples_per_s"] = n * r["mean_iterations"] * (2 * radius + 1) ** 2 / (r["ms_median"] / 1e3)
        res["lk"][str(n)] = r
        print("lk", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
