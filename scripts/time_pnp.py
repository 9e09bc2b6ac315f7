"""GPU times of EPnP and of the local optimisation of the P3P RANSAC (csrc/epnp.hip) on synthetic scenes; writes
profiles/pnp_times.json.  Two shapes, each a median of --reps windows between device events after a warm-up:
  epnp_solve   vggp_epnp_solve at B = 199 * 50 problems (the reference's local_refinement: 199 frame pairs x lo_num = 50) of
               N = 2048 matches, shared 3-D points, half of the matches masked out, all four candidates
  epnp_lo      vggp_epnp_lo at F = 200 * 30 virtual frames (200 frames x COLMAP's 30 focal length factors) of P = 4096
               points, 30 % outliers, max_rounds = 10, started from the true pose disturbed by a thousandth; with the
               histogram of the rounds' outcome (how many frames gained support)
  pose_score   vggp_pose_score of the same frames with L = 4 poses each
  p3p_ransac   vgg_p3p_ransac at F = 20 * 30 = 600 virtual frames of P = 4096 points, 30 % outliers, H = 1024 samples each (the
               default of RANSACOptions.num_hypotheses): the minimal solver of one thread per sample, the scoring of one
               wavefront per sample, the selection
Beside each time: the bytes the launch has to move, computed here from the shapes (the 2-D points of a problem are read
in two sweeps, its mask in three; the shared 3-D points stay in cache), and what rate that makes of the 6.3 TB/s the
MI355X streams at best -- a statement about the traffic, not about the arithmetic, which the 12 x 12 Jacobi of one
wavefront per problem dominates at small N.  No thresholds: the numbers are reported.  Run under its own time limit, e.g.
    timeout -k 10 600 python scripts/time_pnp.py
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 6.3e12


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


def scene(F, P, outliers, seed):
    """F cameras on shared points: X (P,3), xn (F,P,2), pose (F,3,4), everything on the device"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    kw = dict(generator=g, device="cuda", dtype=torch.float64)
    X = torch.rand(P, 3, **kw) * 2 - 1
    q = torch.randn(F, 4, **kw)
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(F, 3, 3)
    t = torch.cat([torch.rand(F, 2, **kw) * 0.6 - 0.3, 3.6 + 0.8 * torch.rand(F, 1, **kw)], 1)
    pc = torch.einsum("fij,pj->fpi", R, X) + t[:, None]
    xn = pc[..., :2] / pc[..., 2:] + 2e-3 * torch.randn(F, P, 2, **kw)
    bad = torch.rand(F, P, generator=g, device="cuda") < outliers
    xn = torch.where(bad[..., None], torch.rand(F, P, 2, **kw) - 0.5, xn)
    return X, xn, torch.cat([R, t[..., None]], 2), bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_times.json"))
    a = ap.parse_args()
    import torch
    from vggsfm_amd import pose
    from vggsfm_amd.two_view_geo import perspective_n_points as PN
    assert torch.cuda.is_available(), "needs an MI355X"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner}

    B, N = 199 * 50, 2048
    X, xn, _, bad = scene(B, N, 0.0, 0)
    masks = torch.rand(B, N, device="cuda") < 0.5
    sol, variant, valid = PN.epnp_solve(X, xn, masks, return_x_cam=False)
    r = windows(lambda: PN.epnp_solve(X, xn, masks, return_x_cam=False), a.reps, a.inner)
    r["bytes"] = B * N * (2 * 16 + 3)
    r["share_of_peak_bandwidth"] = r["bytes"] / (r["ms_median"] * 1e-3) / PEAK_BYTES_PER_S
    r.update(B=B, N=N, valid=int(valid.sum()), winners=torch.bincount(variant.long(), minlength=4).tolist())
    res["epnp_solve"] = r
    print("epnp_solve", json.dumps(r), flush=True)
    del xn, masks, sol

    F, P, L = 200 * 30, 4096, 4
    X, xn, ps, bad = scene(F, P, 0.3, 1)
    thr = torch.full((F,), (6e-3) ** 2, dtype=torch.float64, device="cuda")
    start = ps * (1 + 1e-3 * torch.randn(F, 3, 4, device="cuda", dtype=torch.float64))
    n0, s0, m0 = pose.pose_score(start[:, None], xn, X, None, thr, return_masks=True)
    n0, s0, m0 = n0[:, 0].contiguous(), s0[:, 0].contiguous(), m0[:, 0].contiguous()
    out = pose.epnp_local_optimisation(start, n0, s0, m0, xn, X, None, thr, 10)
    r = windows(lambda: pose.epnp_local_optimisation(start, n0, s0, m0, xn, X, None, thr, 10), a.reps, a.inner)
    r.update(F=F, P=P, max_rounds=10, inliers_in=float(n0.double().mean()), inliers_out=float(out[1].double().mean()),
             frames_that_gained=int((out[1] > n0).sum()), true_inliers=float((~bad).sum(1).double().mean()))
    res["epnp_lo"] = r
    print("epnp_lo", json.dumps(r), flush=True)
    many = torch.stack([start, out[0], ps, start], 1).contiguous()
    r = windows(lambda: pose.pose_score(many, xn, X, None, thr), a.reps, a.inner)
    r["bytes"] = F * L * P * 16
    r["share_of_peak_bandwidth"] = r["bytes"] / (r["ms_median"] * 1e-3) / PEAK_BYTES_PER_S
    r.update(F=F, P=P, L=L)
    res["pose_score"] = r
    print("pose_score", json.dumps(r), flush=True)
    del many, start, out, xn
    F, P, H = 20 * 30, 4096, 1024
    X, xn, ps, bad = scene(F, P, 0.3, 2)
    thr = torch.full((F,), (6e-3) ** 2, dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    samples = pose.draw_minimal_samples(torch.ones(F, P, dtype=torch.bool, device="cuda"), H, g)
    _, num, _, _, _ = pose.p3p_ransac(xn, X, None, samples, thr)
    r = windows(lambda: pose.p3p_ransac(xn, X, None, samples, thr), a.reps, a.inner)
    r.update(F=F, P=P, H=H, inliers=float(num.double().mean()), true_inliers=float((~bad).sum(1).double().mean()))
    res["p3p_ransac"] = r
    print("p3p_ransac", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
