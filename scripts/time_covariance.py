"""GPU times of the covariance entries (csrc/covariance.hip); writes profiles/covariance_times.json.  Medians of --reps windows
of --inner calls between device events after a warm-up, min .. max beside:
  spd_inverse     vggc_spd_inverse at n = 1202, 3200 and 6002 (the reduced systems of the 200-, 400- and 1000-frame
                  configurations) beside vgg_cholesky_solve (right-hand side behind the matrix: the single-launch form) at the
                  same n in the same run.  Both work in place, so every call is preceded by a device copy of the matrix, timed
                  by itself and reported (`copy_ms`; not subtracted).  Flop model: n^3 / 3 each for the factorisation, the
                  triangular inverse and the product.
  ba_covariance   vggc_ba_covariance on the 200 x 100 k scene of bench.py's default workload (SIMPLE_RADIAL, shared camera,
                  n = 1202) with cameras only and with the points' blocks, beside one LM iteration of the same problem in
                  the same run (the phase loop bench.py times: the first five iterations of a solve between two events,
                  its begin outside them).  The entry synchronises the stream once at its start.
No thresholds: the numbers are reported.  Run under its own time limit, e.g.
    timeout -k 10 600 python scripts/time_covariance.py
"""
import argparse
import ctypes
import json
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--sizes", default="1202,3200,6002")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--tracks", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance_times.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from vggsfm_amd import _lib
    from vggsfm_amd import ba as BA
    from vggsfm_amd.ba_options import BundleAdjustmentOptions
    from vggsfm_amd.dist import ShardedBA
    from vggsfm_amd.scene import make_scene, perturb_for_ba
    assert torch.cuda.is_available(), "needs an MI355X"
    L = _lib.lib()
    st = _lib.stream_ptr
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "spd_inverse": {}}

    for n in (int(v) for v in a.sizes.split(",")):
        g = torch.Generator(device="cuda").manual_seed(n)
        G = torch.randn(n, n, generator=g, device="cuda", dtype=torch.float64)
        A = G @ G.T / n + torch.eye(n, device="cuda", dtype=torch.float64)
        del G
        work = torch.empty(n * n + n, dtype=torch.float64, device="cuda")
        ws_inv = torch.empty(L.vggc_spd_inverse_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        ws_chol = torch.empty(L.vgg_cholesky_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        fail = torch.zeros(1, dtype=torch.int32, device="cuda")
        M = work[:n * n].view(n, n)

        def load():
            M.copy_(A)
            work[n * n:].zero_()

        def inverse():
            load()
            _lib.check(L.vggc_spd_inverse(work, n, ws_inv, fail, st()), "vggc_spd_inverse")

        def factor():
            load()
            _lib.check(L.vgg_cholesky_solve(work, work[n * n:], n, ws_chol, fail, st()), "vgg_cholesky_solve")

        inverse()
        resid = float((A @ M - torch.eye(n, device="cuda", dtype=torch.float64)).abs().max())
        r = {"n": n, "copy_ms": windows(load, a.reps, a.inner)["ms_median"], "cholesky_solve": windows(factor, a.reps, a.inner),
             "spd_inverse": windows(inverse, a.reps, a.inner), "max_abs_A_X_minus_I": resid, "failed": int(fail.item()),
             "gflop_model": n ** 3 / 1e9}
        r["inverse_over_factorisation"] = (r["spd_inverse"]["ms_median"] - r["copy_ms"]) / (r["cholesky_solve"]["ms_median"] - r["copy_ms"])
        res["spd_inverse"][str(n)] = r
        print("spd_inverse", json.dumps(r), flush=True)
        del A, work, ws_inv, ws_chol, M

    S, N = a.frames, a.tracks
    sc = make_scene(S, N, "SIMPLE_RADIAL", shared_camera=True, seed=0, track_seed=1000)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=0)
    D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    prob, _, _ = BA.compile_problem(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), D(extra0), True, "SIMPLE_RADIAL",
                                    camera_split=True, sort_points=BA.SORT_POINTS)
    opts = BundleAdjustmentOptions()
    so = opts.solver_options
    so.max_num_iterations = 25
    so.function_tolerance = so.gradient_tolerance = so.parameter_tolerance = -1.0
    init = [t.clone() for t in (prob.cam_q, prob.cam_t, prob.intr, prob.pts)]
    solver = ShardedBA(prob, opts, 0, 1)

    def begin():
        for dst, src in zip((prob.cam_q, prob.cam_t, prob.intr, prob.pts), init):
            dst.copy_(src)
        solver.begin()

    # the iterations alone: the state reset and ShardedBA.begin (with its host synchronisation) lie outside the events
    K, ts = 5, []
    begin()
    for _ in range(K):
        solver.iteration()
    for _ in range(a.reps):
        begin()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(K):
            solver.iteration()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / K)
    r = {"frames": S, "tracks": N, "observations": int(prob.num_obs), "points": int(prob.pts.shape[0]), "n": 6 * S + 2,
         "lm_iteration": {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "iterations_per_window": K}}
    for dst, src in zip((prob.cam_q, prob.cam_t, prob.intr, prob.pts), init):
        dst.copy_(src)
    cp, co = prob.c_struct(), BA._c_options(opts, overlap=False)
    C, P, n = S, int(prob.pts.shape[0]), 6 * S + 2
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    pose, intr, pi, pts = new(C, 6, 6), new(1, 2, 2), new(C, 6, 2), new(P, 3, 3)
    fail = torch.zeros(1, dtype=torch.int32, device="cuda")
    for key, flags in (("cameras", 1), ("cameras_and_points", 3)):
        nbytes = L.vggc_ba_covariance_workspace_bytes(ctypes.byref(cp), ctypes.byref(co), flags)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        fn = lambda: _lib.check(L.vggc_ba_covariance(ctypes.byref(cp), ctypes.byref(co), ws, nbytes, flags, None, pose, intr, pi,
                                                     pts if flags & 2 else None, fail, st()), "vggc_ba_covariance")
        r[key] = windows(fn, a.reps, a.inner)
        r[key]["workspace_mb"] = nbytes / 2 ** 20
    r["failed"] = int(fail.item())
    r["median_pose_sigma"] = float(torch.diagonal(pose[2:], dim1=1, dim2=2).sqrt().median())
    r["median_point_sigma"] = float(torch.diagonal(pts, dim1=1, dim2=2).clamp(min=0).sqrt().median())
    res["ba_covariance"] = r
    print("ba_covariance", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
