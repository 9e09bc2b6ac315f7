"""GPU times of the 5-point essential-matrix LO-RANSAC (csrc/essential.hip) on synthetic matches; writes
profiles/essential_times.json.  One shape, a 200-frame video's worth of pairs: B = 199 pairs, N = 2048 matches,
H = 1024 samples, lo_num = 50; 30 % outliers, 0.5 px noise, focal lengths that differ per pair.  Each figure is a median of
--reps windows between device events after a warm-up:
  estimate_essential   the whole Python call with a fixed sample table
  five_point           vgge_emat_five_point alone (B x H solves)
  score                vgge_emat_score on its 10 H candidates per pair
  refine               vgge_emat_refine on the lo_num best
No thresholds: the numbers are reported.  Run under its own time limit, e.g.
    timeout -k 10 600 python scripts/time_essential.py
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N, H, LO_NUM = 199, 2048, 1024, 50


def inputs(seed=0):
    import numpy as np
    import torch
    from tests import essential_cases as EC
    rng = np.random.default_rng(seed)
    focal = rng.uniform(700, 1500, (B, 1)) * np.ones((1, 4))
    pp = rng.uniform(300, 700, (B, 4))
    scenes = [EC.two_view_scene(rng, N, focal[b], pp[b], noise=0.5, outliers=0.3) for b in range(B)]
    samples = np.array([rng.choice(N, 5, replace=False) for _ in range(H)], np.int32)
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return D(np.stack([s[0] for s in scenes])), D(np.stack([s[1] for s in scenes])), D(focal), D(pp), samples


def windows(fn, reps):
    """median / min / max milliseconds per call over `reps` windows between device events"""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essential_times.json"))
    args = ap.parse_args()
    import torch
    from vggsfm_amd import _lib
    from vggsfm_amd.two_view_geo import essential as ES
    px1, px2, focal, pp, samples = inputs()
    L = _lib.lib()
    p1, p2 = ES._normalise(px1, px2, focal, pp)
    thr = ((4.0 / focal.mean(dim=-1)) ** 2).contiguous()
    smp = torch.as_tensor(samples, dtype=torch.int32, device="cuda")
    Ea, va = ES._five_point(L, p1, p2, smp)
    cnt, _ = ES._score(L, p1, p2, Ea, va, thr)
    order = torch.sort(cnt, dim=1, descending=True, stable=True).indices[:, :LO_NUM].to(torch.int32).contiguous()
    out = {"shape": {"pairs": B, "matches": N, "samples": H, "lo_num": LO_NUM},
           "device": torch.cuda.get_device_name(0),
           "estimate_essential": windows(lambda: ES.estimate_essential(px1, px2, focal, pp, max_ransac_iters=H, lo_num=LO_NUM,
                                                                       samples=samples), args.reps),
           "five_point": windows(lambda: ES._five_point(L, p1, p2, smp), args.reps),
           "score": windows(lambda: ES._score(L, p1, p2, Ea, va, thr), args.reps),
           "refine": windows(lambda: ES._refine(L, p1, p2, Ea, cnt, order, thr), args.reps)}
    E, num, _ = ES.estimate_essential(px1, px2, focal, pp, max_ransac_iters=H, lo_num=LO_NUM, samples=samples)
    out["median_inliers"] = float(num.double().median())
    print(json.dumps(out))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
