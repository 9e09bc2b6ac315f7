"""GPU times of the masked multi-view triangulation (csrc/multiview.hip) on synthetic tracks; writes
profiles/multiview_times.json.  Two shapes: configs[2]'s (100,000 tracks x 200 views) and a mid one (20,000 x 50);
float32 observations with 1e-3 noise, a bool mask that keeps half the views.  Per shape, each a median of --reps windows
between device events after a warm-up, every window holding --inner back-to-back calls (the short kernels would otherwise
be timed by their launch):
  lean            triangulate_tracks_masked (solve + cheirality + reduced angles + flag), the whole Python call
  solve_entry     vggx_multiview_triangulate with angle_mode 0 (ONE kernel), with the bytes it has to move -- observations,
                  weights, points, flags; computed here from the shapes -- and the rate that makes of the 6.3 TB/s the
                  MI355X streams at best
  angle_entry     vggx_max_tri_angle (the centres and the reduced pass: S (S-1) / 2 pairs per point)
  local_refinement_tri   all tracks x lo_num = 50 candidates of H = 50 hypotheses, shared cameras
and beside each the same work in plain torch ops on the same GPU (the reference itself needs its own tree): the solve as
the reference's einsum / eigh chain; the angles as its (n, S*S) table reduced with max, in chunks of points that fit
1 GiB; local refinement as its `low_mem` loop, timed on --torch-lr-candidates of the 50 candidates and --torch-lr-tracks
of the tracks and reported as measured, with the fraction (it is proportional to both; nothing is extrapolated here).
No thresholds: the numbers are reported.  Run under its own time limit, e.g.
    timeout -k 10 900 python scripts/time_multiview.py
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"configs2": dict(S=200, N=100000), "mid": dict(S=50, N=20000)}
PEAK_BYTES_PER_S = 6.3e12
LO_NUM = H = 50


def inputs(S, N, seed=0):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    ext = torch.zeros(S, 3, 4, dtype=torch.float64, device="cuda")
    ext[:, :, :3] = torch.eye(3, dtype=torch.float64, device="cuda")
    u = torch.rand(S, 3, generator=g, device="cuda", dtype=torch.float64)
    ext[:, 0, 3], ext[:, 1, 3], ext[:, 2, 3] = -(u[:, 0] * 4 - 2), -(u[:, 1] * 2 - 1), 5 - (u[:, 2] - 0.5)
    X = torch.rand(N, 3, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    cam = X[None] + ext[:, None, :, 3]
    tracks = (cam[..., :2] / cam[..., 2:] + 1e-3 * torch.randn(S, N, 2, generator=g, device="cuda", dtype=torch.float64)).float()
    keep = torch.rand(S, N, generator=g, device="cuda") < 0.5
    return ext, tracks, keep


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


def torch_solve(ext, tracks, w):
    import torch
    h = torch.cat([tracks, torch.ones_like(tracks[..., :1])], -1)
    r = h / h.norm(dim=-1, keepdim=True)
    terms = ext[:, None] - r[..., :, None] * torch.einsum("sni,sik->snk", r, ext)[:, :, None, :]
    terms = terms * w[:, :, None, None]
    A = torch.einsum("snij,snik->njk", terms, terms)
    v = torch.linalg.eigh(A)[1][:, :, 0]
    X = v[:, :3] / v[:, 3:]
    z = torch.einsum("sj,nj->ns", ext[:, 2, :3], X) + ext[None, :, 2, 3]
    return X, (z <= 0).any(1)


def torch_max_angle(centers, P, thr, any_only=False):
    import torch
    S = centers.shape[0]
    step = max(1, (1 << 30) // (8 * S * S))
    bsq = (centers[:, None] - centers[None]).norm(dim=-1) ** 2
    out = []
    for a in range(0, len(P), step):
        r = (P[a:a + step, None] - centers[None]).norm(dim=-1) ** 2
        den = 2.0 * torch.sqrt(r[:, :, None] * r[:, None, :])
        nom = r[:, :, None] + r[:, None, :] - bsq[None]
        bad = den <= 1e-12
        th = torch.acos(torch.clamp(torch.where(bad, torch.ones_like(nom), nom) / torch.where(bad, torch.ones_like(den), den),
                                    -1.0, 1.0)).abs()
        th = torch.min(th, torch.pi - th) * (180.0 / torch.pi)
        out.append((th >= thr).flatten(1).any(1) if any_only else th.flatten(1).max(1).values)
    return torch.cat(out)


def gpu(a):
    import torch

    from vggsfm_amd import _lib
    from vggsfm_amd.utils import triangulation as TR
    from vggsfm_amd.utils import triangulation_helpers as TH

    L = _lib.lib()
    res = {"reps": a.reps, "inner": a.inner, "peak_bytes_per_s": PEAK_BYTES_PER_S, "lo_num": LO_NUM, "shapes": {}}
    for name in a.shapes:
        S, N = SHAPES[name]["S"], SHAPES[name]["N"]
        ext, tracks, keep = inputs(S, N)
        r = {"S": S, "N": N}
        pts, valid, ang, flag = TR.triangulate_tracks_masked(ext, tracks, keep, 1.5)
        r["lean"] = windows(lambda: TR.triangulate_tracks_masked(ext, tracks, keep, 1.5), a.reps, a.inner)
        # the solve kernel alone
        w8 = keep.contiguous().view(torch.uint8)
        out_p = torch.empty((N, 3), dtype=torch.float64, device="cuda")
        out_i = torch.empty(N, dtype=torch.uint8, device="cuda")
        st = _lib.stream_ptr()

        def solve():
            _lib.check(L.vggx_multiview_triangulate(ext, 1, 1, tracks, 0, 2, 2 * N, w8, 1, 1, N, None, N, S, 0, 0, 0.0, out_p, out_i,
                                                    None, None, None, st), "vggx_multiview_triangulate")
        r["solve_entry"] = windows(solve, a.reps, a.inner)
        assert torch.equal(out_p, pts)
        nbytes = N * S * (8 + 1) + N * (24 + 1) + S * 96
        rate = nbytes / (r["solve_entry"]["ms_median"] * 1e-3)
        r["solve_entry"].update(bytes=nbytes, bytes_per_s=rate, share_of_peak_bandwidth=rate / PEAK_BYTES_PER_S)
        # the reduced angle pass alone
        out_a = torch.empty(N, dtype=torch.float64, device="cuda")
        out_f = torch.empty(N, dtype=torch.uint8, device="cuda")
        ws = torch.empty(L.vggx_multiview_workspace_bytes(1, S), dtype=torch.uint8, device="cuda")

        def angles():
            _lib.check(L.vggx_max_tri_angle(ext, 1, 1, pts, N, S, 1, 1.5, out_a, out_f, ws, st), "vggx_max_tri_angle")
        r["angle_entry"] = windows(angles, a.reps, max(1, a.inner // 4))
        r["angle_entry"]["pairs_per_point"] = S * (S - 1) // 2
        assert torch.equal(out_a, ang)
        # the same in torch
        t64, w64 = tracks.double(), keep.double()
        Xt, _ = torch_solve(ext, t64, w64)
        r["solve_max_rel_deviation_from_torch"] = ((pts - Xt).norm(dim=1) / Xt.norm(dim=1)).max().item()
        r["torch_solve"] = windows(lambda: torch_solve(ext, t64, w64), max(3, a.reps // 2), 1)
        centers = -torch.einsum("sji,sj->si", ext[:, :, :3], ext[:, :, 3])
        r["torch_max_angle"] = windows(lambda: torch_max_angle(centers, pts, 1.5), 3, 1)
        del Xt, t64, w64
        # local refinement: every track, lo_num candidates out of H hypotheses of random inlier sets
        g = torch.Generator(device="cuda").manual_seed(1)
        inl = torch.rand(N, H, S, generator=g, device="cuda") < 0.5
        order = torch.argsort(torch.rand(N, H, generator=g, device="cuda"), dim=1)
        p1 = tracks.permute(1, 0, 2).contiguous()
        cams = ext[None].expand(N, -1, -1, -1)
        lr = TH.local_refinement_tri(p1, cams, 1.5, inl, order, lo_num=LO_NUM)
        r["local_refinement_tri"] = windows(lambda: TH.local_refinement_tri(p1, cams, 1.5, inl, order, lo_num=LO_NUM), a.reps, 1)
        r["local_refinement_tri"]["solves"] = N * LO_NUM
        nt, nc = max(1, int(N * a.torch_lr_tracks)), a.torch_lr_candidates
        p1d = p1[:nt].double().permute(1, 0, 2).contiguous()

        def torch_lr():
            for k in range(nc):
                m = inl[torch.arange(nt, device="cuda"), order[:nt, k]].t().double()             # (S,nt)
                X, _ = torch_solve(ext, p1d * m[..., None], m)
                torch_max_angle(centers, X, 1.5, any_only=True)
        r["torch_local_refinement_subset"] = windows(torch_lr, 3, 1)
        r["torch_local_refinement_subset"].update(tracks=nt, candidates=nc, fraction_of_the_work=nt * nc / (N * LO_NUM))
        res["shapes"][name] = r
        print(name, json.dumps(r), flush=True)
        del inl, order, p1, lr, cams, p1d
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--torch-lr-candidates", type=int, default=2)
    ap.add_argument("--torch-lr-tracks", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiview_times.json"))
    a = ap.parse_args()
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res = gpu(a)
    shapes = dict(old.get("shapes", {}), **res["shapes"])
    old.update(res)
    old["shapes"] = shapes
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(old, f, indent=1)
        f.write("\n")
    print(json.dumps(old))


if __name__ == "__main__":
    main()
