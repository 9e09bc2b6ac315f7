"""GPU times of the Sim(3) and pose-error entries (csrc/sim3.hip); writes profiles/sim3_times.json.  Medians of --reps windows
of --inner calls between device events after a warm-up, min .. max beside, each beside a torch formulation of the same
computation on the same device in the same run:
  ransac        vggs_sim3_ransac at B = 1, N = 250 k, H = 1024, lo_rounds = 10 and at B = 64, N = 1024, H = 256 (30 % outliers,
                max_error = 5 sigma).  torch: batched 3-point Umeyama (torch.linalg.svd), residuals of all points under a chunk
                of hypotheses at a time (chunked so that the (B, chunk, N, 3) tensor fits), the same ranking, and every LO
                round evaluated with the accept rule as torch.where (the kernels turn a stopped problem's rounds into no-ops
                on the device; neither side returns to the host)
  fit           vggs_sim3_fit at N = 250 k beside a torch Umeyama
  score         vggs_sim3_score alone at N = 250 k, H = 1024, with the byte and flop model of DESIGN.md section 20: the points
                are streamed ceil(H / 32) times (48 bytes per point and stream), 31 flops per point and hypothesis
  pair_errors   vggs_pose_pair_errors at S = 1000 and S = 5000 beside the reference's camera_to_rel_deg arithmetic
                (vggsfm_amd/utils/metric.py: 4 x 4 matrices per pair, closed-form inverse, bmm, quaternions)
No thresholds: the numbers are reported.  Run under its own time limit, e.g.
    timeout -k 10 600 python scripts/time_sim3.py
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK, FP64_PEAK = 8.0e12, 78.6e12
TILE, FLOPS_PER_PAIR, BYTES_PER_POINT = 32, 31, 48


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


def torch_umeyama(src, tgt, w):
    """(..., N, 3) points, (..., N) weights -> (s (...), R (...,3,3), t (...,3)); no validity rules."""
    import torch
    W = w.sum(-1, keepdim=True)
    mu_s, mu_t = (w[..., None] * src).sum(-2) / W, (w[..., None] * tgt).sum(-2) / W
    ds, dt = src - mu_s[..., None, :], tgt - mu_t[..., None, :]
    Sigma = (w[..., None] * dt).transpose(-1, -2) @ ds / W[..., None]
    var = (w * (ds * ds).sum(-1)).sum(-1) / W[..., 0]
    U, S, Vh = torch.linalg.svd(Sigma)
    d = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vh))
    D = torch.ones_like(S)
    D[..., 2] = d
    R = (U * D[..., None, :]) @ Vh
    s = (S * D).sum(-1) / var
    t = mu_t - s[..., None] * (R @ mu_s[..., None])[..., 0]
    return s, R, t


def torch_score(src, tgt, s, R, t, thr2, chunk):
    """src, tgt (B,N,3); s (B,H), R (B,H,3,3), t (B,H,3) -> counts (B,H), sums (B,H), hypotheses in chunks"""
    import torch
    counts, sums = [], []
    for h0 in range(0, s.shape[1], chunk):
        y = torch.einsum("bhij,bnj->bhni", R[:, h0:h0 + chunk], src) * s[:, h0:h0 + chunk, None, None] + t[:, h0:h0 + chunk, None]
        r = ((tgt[:, None] - y) ** 2).sum(-1)
        inl = r <= thr2[:, None, None]
        counts.append(inl.sum(-1))
        sums.append((r * inl).sum(-1))
    return torch.cat(counts, 1), torch.cat(sums, 1)


def torch_ransac(src, tgt, samples, thr2, lo_rounds, chunk):
    import torch
    B, N, _ = src.shape
    idx = samples.long()
    ar = torch.arange(B, device=src.device)[:, None, None]
    s, R, t = torch_umeyama(src[ar, idx], tgt[ar, idx], torch.ones(idx.shape, dtype=src.dtype, device=src.device))
    ok = (idx[..., 0] != idx[..., 1]) & (idx[..., 0] != idx[..., 2]) & (idx[..., 1] != idx[..., 2]) & torch.isfinite(s)
    counts, sums = torch_score(src, tgt, torch.nan_to_num(s), torch.nan_to_num(R), torch.nan_to_num(t), thr2, chunk)
    counts = torch.where(ok, counts, torch.full_like(counts, -1))
    top = counts.max(1, keepdim=True).values
    best = torch.where(counts == top, sums, torch.full_like(sums, float("inf"))).argmin(1)
    b = torch.arange(B, device=src.device)
    cs, cR, ct, cc, cq = s[b, best], R[b, best], t[b, best], counts[b, best], sums[b, best]
    for _ in range(lo_rounds):
        r = ((tgt - (cs[:, None, None] * (src @ cR.transpose(1, 2)) + ct[:, None])) ** 2).sum(-1)
        w = (r <= thr2[:, None]).to(src.dtype)
        ns, nR, nt = torch_umeyama(src, tgt, w)
        nc, nq = torch_score(src, tgt, ns[:, None], nR[:, None], nt[:, None], thr2, 1)
        better = (nc[:, 0] > cc) | ((nc[:, 0] == cc) & (nq[:, 0] < cq))
        cs, cR, ct = torch.where(better, ns, cs), torch.where(better[:, None, None], nR, cR), torch.where(better[:, None], nt, ct)
        cc, cq = torch.where(better, nc[:, 0], cc), torch.where(better, nq[:, 0], cq)
    return cs, cR, ct, cc


def scene(B, N, seed, sigma=1e-3):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *shape: torch.rand(*shape, generator=g, device="cuda", dtype=torch.float64)
    src = 2 * rnd(B, N, 3) - 1
    Q, _ = torch.linalg.qr(torch.randn(B, 3, 3, generator=g, device="cuda", dtype=torch.float64))
    Q = Q * torch.sign(torch.linalg.det(Q))[:, None, None]
    tgt = 2.0 * src @ Q.transpose(1, 2) + torch.randn(B, 1, 3, generator=g, device="cuda", dtype=torch.float64)
    tgt = tgt + sigma * torch.randn(B, N, 3, generator=g, device="cuda", dtype=torch.float64)
    bad = rnd(B, N) < 0.3
    tgt = torch.where(bad[..., None], 6 * rnd(B, N, 3) - 3, tgt)
    return src.contiguous(), tgt.contiguous(), torch.full((B,), 5 * sigma, dtype=torch.float64, device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--points", type=int, default=250000)
    ap.add_argument("--cameras", default="1000,5000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_times.json"))
    a = ap.parse_args()
    import torch
    from vggsfm_amd import _lib, sim3
    from vggsfm_amd.utils import metric
    assert torch.cuda.is_available(), "needs an MI355X"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "ransac": {}, "pair_errors": {}}
    ratio = lambda r: r["torch"]["ms_median"] / r["hip"]["ms_median"]

    for key, (B, N, H, lo, chunk) in {"B1_N250k_H1024_lo10": (1, a.points, 1024, 10, 64), "B64_N1024_H256": (64, 1024, 256, 10, 64)}.items():
        src, tgt, err = scene(B, N, seed=B)
        samples = torch.randint(0, N, (B, H, 3), device="cuda", dtype=torch.int32)
        ws = torch.empty(int(_lib.lib().vggs_sim3_workspace_bytes(B, N, H)), dtype=torch.uint8, device="cuda")
        hip = lambda: sim3.estimate_sim3_robust(src, tgt, err, samples=samples, lo_rounds=lo, workspace=ws)
        ref = lambda: torch_ransac(src, tgt, samples, err * err, lo, chunk)
        out, cmp = hip(), ref()
        r = {"B": B, "N": N, "H": H, "lo_rounds": lo, "hip": windows(hip, a.reps, a.inner), "torch": windows(ref, a.reps, a.inner),
             "torch_chunk": chunk, "inliers_hip": out[3].tolist()[:4], "inliers_torch": cmp[3].tolist()[:4],
             "workspace_mb": ws.numel() / 2 ** 20}
        r["torch_over_hip"] = ratio(r)
        res["ransac"][key] = r
        print("ransac", key, json.dumps(r), flush=True)
        if B == 1:
            w = torch.ones(B, N, dtype=torch.float64, device="cuda")
            f = {"N": N, "hip": windows(lambda: sim3.estimate_sim3(src, tgt), a.reps, a.inner),
                 "torch": windows(lambda: torch_umeyama(src, tgt, w), a.reps, a.inner)}
            f["torch_over_hip"] = ratio(f)
            res["fit"] = f
            print("fit", json.dumps(f), flush=True)
            s, R, t = (x[:, None].expand((B, H) + tuple(x.shape[1:])).contiguous() for x in (out[0], out[1], out[2]))
            valid = torch.ones(B, H, dtype=torch.uint8, device="cuda")
            sc = {"N": N, "H": H, "hip": windows(lambda: sim3.score_sim3(src, tgt, s, R, t, valid, err), a.reps, a.inner),
                  "torch": windows(lambda: torch_score(src, tgt, s, R, t, err * err, chunk), a.reps, a.inner)}
            streams = math.ceil(H / TILE)
            sec = sc["hip"]["ms_median"] / 1e3
            sc.update(point_streams=streams, bytes_model=streams * N * BYTES_PER_POINT, flops_model=N * H * FLOPS_PER_PAIR)
            sc.update(bytes_per_s=sc["bytes_model"] / sec, flops_per_s=sc["flops_model"] / sec,
                      share_of_hbm_peak=sc["bytes_model"] / sec / HBM_PEAK, share_of_fp64_peak=sc["flops_model"] / sec / FP64_PEAK)
            sc["torch_over_hip"] = ratio(sc)
            res["score"] = sc
            print("score", json.dumps(sc), flush=True)
        del src, tgt, ws

    class Cameras:
        def __init__(self, P):
            self.M = torch.zeros(len(P), 4, 4, dtype=P.dtype, device=P.device)
            self.M[:, :3, :3] = P[:, :, :3].transpose(1, 2)
            self.M[:, 3, :3] = P[:, :, 3]
            self.M[:, 3, 3] = 1

        def get_world_to_view_transform(self):
            return self

        def get_matrix(self):
            return self.M

    for S in (int(v) for v in a.cameras.split(",")):
        g = torch.Generator(device="cuda").manual_seed(S)
        Q, _ = torch.linalg.qr(torch.randn(S, 3, 3, generator=g, device="cuda", dtype=torch.float64))
        Q = Q * torch.sign(torch.linalg.det(Q))[:, None, None]
        gt = torch.cat([Q, torch.randn(S, 3, 1, generator=g, device="cuda", dtype=torch.float64)], dim=2).contiguous()
        pred = gt + 0.01 * torch.randn(S, 3, 4, generator=g, device="cuda", dtype=torch.float64)
        cg, cp = Cameras(gt), Cameras(pred)
        r = {"S": S, "pairs": S * (S - 1) // 2, "hip": windows(lambda: metric.pose_pair_errors(pred, gt), a.reps, a.inner),
             "torch": windows(lambda: metric.camera_to_rel_deg(cp, cg, "cuda", 1), a.reps, a.inner)}
        r["torch_over_hip"] = ratio(r)
        res["pair_errors"][str(S)] = r
        print("pair_errors", json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
