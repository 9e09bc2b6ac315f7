"""Writes tests/golden/multiview_<case>.npz: inputs and the float64 outputs of the reference's own
``triangulate_multi_view_point_batched``, ``calculate_triangulation_angle_batched`` / ``_exhaustive`` / ``calculate_triangulation_angle``,
``calculate_normalized_angular_error_batched``, ``local_refinement_tri`` (vggsfm/utils/triangulation_helpers.py) and
``triangulate_multi_view_point_from_tracks`` (vggsfm/utils/triangulation.py), imported through oracle.ref_harness and run on
the CPU in float64.  The files are written with fixed zip time stamps: the same script gives the same bytes.

  python scripts/make_golden_multiview.py [case ...]

Admission -- what a test may compare -- is decided here, from the reference alone, and stored with the outputs:
  admit_points   the reference's own point moves by less than 1e-10 (relative, 2-norm) when every observation is jittered by
                 1e-13 relative (fixed seed): its conditioning, not the device's arithmetic, is what a comparison would see
  admit_che      every view's depth z of the reference's point is at least 1e-6 away from 0 (and the point is admitted)
  admit_flag     the largest angle of the reference's table is at least 1e-6 degrees away from min_tri_angle (same)
  angles         of admitted points only; compared as angles where the cosine is <= 1 - 1e-6 and as cosines elsewhere
                 (tests/multiview_cases.py: `angle_deviation`)
No file may leave out more than 2 % of its points, booleans or angles: asserted when the file is written.

Cases (S views, N points; cameras look roughly down +z at a unit cube 5 away; observation noise 1e-3):
  bool_s8        bool mask, about half the views of every point
  float_s8       float weights in (0.2, 1.5) with exact zeros
  nomask_s6      no mask
  two_views      S = 2
  many_s24       S = 24, bool mask
  behind_s6      one camera stands inside the cube looking away: masked out for every point, yet it decides cheirality
  coincident_s5  cameras 1 and 3 share their centre (baseline 0: the cosine of that pair is 1); view 0 is kept for every point
  f32_s8         float32 observations, bool mask
  from_tracks    triangulate_multi_view_point_from_tracks with B = 1, bool mask
  lr_lo1 / lr_lo50   local_refinement_tri with lo_num 1 / 50: per-track cameras whose baselines subtend about 1 .. 45 degrees
  angles         the three angle functions on given points: per-point cameras, a point AT a camera centre (the eps branch),
                 coincident centres, a non-default eps
  angerr         calculate_normalized_angular_error_batched, radians and degrees, with a ray pair of cosine exactly 1
"""
import io
import os
import sys
import warnings
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
JITTER, POINT_MOVE, CLEAR, CAP = 1e-13, 1e-10, 1e-6, 0.02

TRI_CASES = {
    "bool_s8": dict(S=8, N=300, seed=101, mask="bool"),
    "float_s8": dict(S=8, N=300, seed=102, mask="float"),
    "nomask_s6": dict(S=6, N=300, seed=103, mask=None),
    "two_views": dict(S=2, N=300, seed=104, mask=None),
    "many_s24": dict(S=24, N=96, seed=105, mask="bool"),
    "behind_s6": dict(S=6, N=300, seed=106, mask="bool", behind=True),
    "coincident_s5": dict(S=5, N=300, seed=107, mask="bool", coincident=True),
    "f32_s8": dict(S=8, N=300, seed=108, mask="bool", f32=True),
}
LR_CASES = {"lr_lo1": dict(B=48, N=10, H=60, lo_num=1, seed=121), "lr_lo50": dict(B=48, N=10, H=60, lo_num=50, seed=122)}
MIN_TRI_ANGLE = 1.5


def rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def cameras(rng, S, spread=1.0):
    ext = np.zeros((S, 3, 4))
    for s in range(S):
        c = np.array([rng.uniform(-2, 2) * spread, rng.uniform(-1, 1) * spread, -5 + rng.uniform(-0.5, 0.5) * spread])
        R = rodrigues(rng.uniform(-0.1, 0.1, 3) + 1e-3)
        ext[s, :, :3], ext[s, :, 3] = R, -R @ c
    return ext


def observe(rng, ext, X, noise=1e-3):
    """ext (S,3,4), X (N,3) -> (S,N,2) normalised observations with noise"""
    cam = np.einsum("sij,nj->sni", ext[:, :, :3], X) + ext[:, None, :, 3]
    return cam[..., :2] / cam[..., 2:3] + noise * rng.standard_normal(cam[..., :2].shape)


def view_mask(rng, kind, S, N):
    if kind is None:
        return None
    keep = rng.uniform(size=(S, N)) < 0.55
    for n in range(N):                                    # at least two views each (fewer has no defined answer)
        while keep[:, n].sum() < 2:
            keep[rng.integers(S), n] = True
    if kind == "bool":
        return keep
    return np.where(keep, rng.uniform(0.2, 1.5, size=(S, N)), 0.0)


def jitter(rng, a):
    return a * (1.0 + JITTER * rng.standard_normal(a.shape))


def capped(name, what, admit):
    left = 1.0 - float(np.mean(admit)) if admit.size else 0.0
    assert left <= CAP, f"{name}: {100 * left:.2f} % of the {what} left out (cap {100 * CAP:.0f} %)"
    return left


def admit_points(ref, moved):
    rel = np.linalg.norm(moved - ref, axis=-1) / np.linalg.norm(ref, axis=-1)
    return rel < POINT_MOVE, float(rel.max())


def depths(ext_per_point, pts):
    """ext (B,S,3,4), pts (B,3) -> z (B,S)"""
    return np.einsum("bsj,bj->bs", ext_per_point[:, :, 2, :3], pts) + ext_per_point[:, :, 2, 3]


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps and member order."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    assert os.path.getsize(path) < 1_000_000, f"{path}: {os.path.getsize(path)} bytes"


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def tri_case(name, c, TH, TR):
    rng = np.random.default_rng(c["seed"])
    S, N = c["S"], c["N"]
    ext = cameras(rng, S)
    if c.get("coincident"):
        centre1 = -ext[1, :, :3].T @ ext[1, :, 3]
        ext[3, :, 3] = -ext[3, :, :3] @ centre1
    if c.get("behind"):
        ext[2, :, :3], ext[2, :, 3] = rodrigues(np.array([0.02, -0.03, 0.01])), -rodrigues(np.array([0.02, -0.03, 0.01])) @ \
            np.array([0.1, -0.1, 0.2])
    X = rng.uniform(-1, 1, size=(N, 3))
    tracks = observe(rng, ext, X)
    mask = view_mask(rng, c["mask"], S, N)
    if c.get("behind"):
        mask[2] = False
        for n in range(N):
            while mask[:, n].sum() < 2:
                mask[rng.choice([0, 1, 3, 4, 5]), n] = True
    if c.get("coincident"):
        mask[0] = True                                        # (views 1 and 3 alone have no parallax)
    if c.get("f32"):
        tracks = tracks.astype(np.float32)
    t64 = tracks.astype(np.float64)

    def run(tr):
        cams = T(ext)[None].expand(N, -1, -1, -1)
        return TH.triangulate_multi_view_point_batched(cams, T(tr).permute(1, 0, 2), None if mask is None else T(mask).t(),
                                                       compute_tri_angle=True, check_cheirality=True)
    pts, ang, inv = (x.numpy() for x in run(tracks))
    assert pts.dtype == np.float64 and ang.dtype == np.float64
    moved = run(jitter(np.random.default_rng(c["seed"] + 5000), t64))[0].numpy()
    ap, worst = admit_points(pts, moved)
    z = depths(np.broadcast_to(ext, (N, S, 3, 4)), pts)
    ac = ap & (np.abs(z).min(1) >= CLEAR)
    af = ap & (np.abs(ang.max(1) - MIN_TRI_ANGLE) >= CLEAR)
    left = [capped(name, "points", ap), capped(name, "cheirality flags", ac), capped(name, "angle flags", af)]
    arrays = dict(extrinsics=ext, tracks=tracks, ref_points=pts, ref_angles=ang, ref_invalid=inv, admit_points=ap,
                  admit_che=ac, admit_flag=af, min_tri_angle=np.float64(MIN_TRI_ANGLE))
    if mask is not None:
        arrays["mask"] = mask
    save_npz(os.path.join(OUT, f"multiview_{name}.npz"), arrays)
    print(f"{name}: jitter moved the reference by <= {worst:.1e}; left out {[f'{100 * x:.2f} %' for x in left]}; "
          f"{int(inv.sum())} of {N} invalid cheirality, max angle {ang.max(1).min():.2f} .. {ang.max():.2f} deg")


def from_tracks_case(TH, TR):
    name, seed, S, N = "from_tracks", 111, 8, 300
    rng = np.random.default_rng(seed)
    ext = cameras(rng, S)
    X = rng.uniform(-1, 1, size=(N, 3))
    tracks = observe(rng, ext, X)
    mask = view_mask(rng, "bool", S, N)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pts, che = (x.numpy() for x in TR.triangulate_multi_view_point_from_tracks(T(ext)[None], T(tracks)[None], T(mask)[None]))
        moved = TR.triangulate_multi_view_point_from_tracks(T(ext)[None], T(jitter(np.random.default_rng(seed + 5000), tracks))[None],
                                                            T(mask)[None])[0].numpy()
    assert pts.dtype == np.float64 and pts.shape == (1, N, 3)
    ap, worst = admit_points(pts[0], moved[0])
    ac = ap & (np.abs(depths(np.broadcast_to(ext, (N, S, 3, 4)), pts[0])).min(1) >= CLEAR)
    left = [capped(name, "points", ap), capped(name, "cheirality flags", ac)]
    save_npz(os.path.join(OUT, f"multiview_{name}.npz"), dict(extrinsics=ext[None], tracks=tracks[None], mask=mask[None],
                                                              ref_points=pts, ref_cheirality=che, admit_points=ap[None],
                                                              admit_che=ac[None]))
    print(f"{name}: jitter moved the reference by <= {worst:.1e}; left out {[f'{100 * x:.2f} %' for x in left]}")


def lr_case(name, c, TH, TR):
    rng = np.random.default_rng(c["seed"])
    B, N, H, lo = c["B"], c["N"], c["H"], c["lo_num"]
    ext = np.stack([cameras(rng, N, spread=10 ** rng.uniform(-1.6, 0)) for _ in range(B)])       # (B,N,3,4)
    X = rng.uniform(-1, 1, size=(B, 3))
    points1 = np.stack([observe(rng, ext[b], X[b:b + 1])[:, 0] for b in range(B)])                # (B,N,2)
    inl = rng.uniform(size=(B, H, N)) < 0.6
    for b in range(B):
        for h in range(H):
            while inl[b, h].sum() < 2:
                inl[b, h, rng.integers(N)] = True
    order = np.stack([rng.permutation(H) for _ in range(B)]).astype(np.int64)

    def run(p1):
        return TH.local_refinement_tri(T(p1), T(ext), MIN_TRI_ANGLE, T(inl), T(order), lo_num=lo)
    pts, flag, inv = (x.numpy() for x in run(points1))
    assert pts.dtype == np.float64 and pts.shape == (B, lo, 3)
    moved = run(jitter(np.random.default_rng(c["seed"] + 5000), points1))[0].numpy()
    ap, worst = admit_points(pts.reshape(-1, 3), moved.reshape(-1, 3))
    ext_q = np.repeat(ext, lo, axis=0)
    table = TH.calculate_triangulation_angle_batched(T(ext_q), T(pts.reshape(-1, 3))).numpy()
    assert ((table >= MIN_TRI_ANGLE).any(1) == flag.reshape(-1)).all()
    af = ap & (np.abs(table.max(1) - MIN_TRI_ANGLE) >= CLEAR)
    ac = ap & (np.abs(depths(ext_q, pts.reshape(-1, 3))).min(1) >= CLEAR)
    left = [capped(name, "points", ap), capped(name, "cheirality flags", ac), capped(name, "angle flags", af)]
    save_npz(os.path.join(OUT, f"multiview_{name}.npz"),
             dict(points1=points1, extrinsics=ext, inlier_mask=inl, sorted_indices=order, lo_num=np.int64(lo),
                  min_tri_angle=np.float64(MIN_TRI_ANGLE), ref_points=pts, ref_tri_angle_masks=flag, ref_invalid=inv,
                  admit_points=ap.reshape(B, lo), admit_che=ac.reshape(B, lo), admit_flag=af.reshape(B, lo)))
    print(f"{name}: jitter moved the reference by <= {worst:.1e}; left out {[f'{100 * x:.2f} %' for x in left]}; "
          f"{int(flag.sum())} of {flag.size} angle flags set, {int(inv.sum())} invalid cheirality")


def angles_case(TH, TR):
    rng = np.random.default_rng(131)
    B, S = 60, 6
    ext_b = np.stack([cameras(rng, S, spread=10 ** rng.uniform(-2, 0)) for _ in range(B)])
    ext_b[:, 4, :, 3] = -np.einsum("bij,bj->bi", ext_b[:, 4, :, :3], -np.einsum("bji,bj->bi", ext_b[:, 1, :, :3], ext_b[:, 1, :, 3]))
    pts_b = rng.uniform(-1, 1, size=(B, 3))
    centre = lambda e: -e[:, :3].T @ e[:, 3]
    pts_b[0] = centre(ext_b[0, 2])                                  # a point AT a camera centre: denominator 0
    eps_b = 1e-12
    batched = TH.calculate_triangulation_angle_batched(T(ext_b), T(pts_b), eps_b).numpy()
    Se, P = 7, 80
    ext_e = cameras(rng, Se)
    ext_e[5, :, 3] = -ext_e[5, :, :3] @ centre(ext_e[2])
    pts_e = rng.uniform(-1, 1, size=(P, 3))
    pts_e[3] = centre(ext_e[4])
    exhaustive = TH.calculate_triangulation_angle_exhaustive(T(ext_e), T(pts_e)).numpy()
    assert exhaustive.shape == (Se * Se, P)
    K = 40
    c1, c2 = rng.uniform(-2, 2, size=(K, 3)), rng.uniform(-2, 2, size=(K, 3))
    c2[7] = c1[7]
    pts_p = rng.uniform(-1, 1, size=(50, 3))
    pts_p[0], pts_p[1] = c1[5], c1[6] + 1e-4                      # r1 = 0; r1 r2 ~ 1e-8 against eps 1e-3: the eps branch
    eps_p = 1e-3
    pairs = TH.calculate_triangulation_angle(T(c1), T(c2), T(pts_p), eps_p).numpy()
    assert batched[0, 2 * S + 3] == 0.0 and exhaustive[4 * Se + 1, 3] == 0.0 and pairs[5, 0] == 0.0
    save_npz(os.path.join(OUT, "multiview_angles.npz"),
             dict(batched_extrinsics=ext_b, batched_points=pts_b, batched_eps=np.float64(eps_b), ref_batched=batched,
                  exhaustive_extrinsics=ext_e, exhaustive_points=pts_e, ref_exhaustive=exhaustive,
                  pairs_center1=c1, pairs_center2=c2, pairs_points=pts_p, pairs_eps=np.float64(eps_p), ref_pairs=pairs))
    print(f"angles: batched {batched.shape}, exhaustive {exhaustive.shape}, pairs {pairs.shape}; "
          f"{int((batched == 0).sum() + (exhaustive == 0).sum() + (pairs == 0).sum())} exact zeros")


def angerr_case(TH, TR):
    rng = np.random.default_rng(141)
    B, N, P = 6, 50, 4
    ext = cameras(rng, B)
    X = rng.uniform(-1, 1, size=(P, N, 3))
    p2 = np.stack([observe(rng, ext, X[0], noise=2e-2)[b] for b in range(B)])                      # (B,N,2)
    cam = ext[1, :, :3] @ X[2, 5] + ext[1, :, 3]
    p2[1, 5] = cam[:2] / cam[2]                                    # the ray through the point itself: cosine 1
    rad, cos = (x.numpy() for x in TH.calculate_normalized_angular_error_batched(T(p2), T(X), T(ext)))
    deg, cos2 = (x.numpy() for x in TH.calculate_normalized_angular_error_batched(T(p2), T(X), T(ext), to_degree=True))
    assert rad.shape == (P, B, N) and (cos == cos2).all()
    save_npz(os.path.join(OUT, "multiview_angerr.npz"), dict(point2D=p2, point3D=X, cam_from_world=ext, ref_rad=rad,
                                                             ref_deg=deg, ref_cos=cos))
    print(f"angerr: {rad.shape}, cos in [{cos.min():.6f}, {cos.max():.17g}]")


def main():
    args = sys.argv[1:]
    TR, TH, _ = ref_harness.load()
    want = lambda n: not args or n in args
    for name, c in TRI_CASES.items():
        if want(name):
            tri_case(name, c, TH, TR)
    if want("from_tracks"):
        from_tracks_case(TH, TR)
    for name, c in LR_CASES.items():
        if want(name):
            lr_case(name, c, TH, TR)
    if want("angles"):
        angles_case(TH, TR)
    if want("angerr"):
        angerr_case(TH, TR)


if __name__ == "__main__":
    main()
