"""Masked multi-view triangulation and its helpers on the GPU (csrc/multiview.hip) against the reference's goldens
(tests/golden/multiview_*.npz) on the admitted set, and the bit-for-bit contracts between the forms.

Bounds (tests/multiview_cases.py, where the rule is written down): largest deviations measured on an MI355X over all goldens
and admitted entries -- points 5.6e-11 relative (lr_lo50), angles 2.4e-11 degrees (behind_s6), cosines 2.2e-16 -- give
POINT_TOL 1e-9, ANGLE_TOL 1e-9, COS_TOL 1e-14: the smallest powers of ten at least 10 x the measured values, capped at 1e-9.
At 100,000 x 200 against torch's eigh on the same device: points 9.3e-14, largest angle 5.0e-14 degrees.  Every test prints
its figures before it asserts."""
import numpy as np
import pytest
import torch

from tests import multiview_cases as MC
from vggsfm_amd.utils import triangulation as TR
from vggsfm_amd.utils import triangulation_helpers as TH

pytestmark = pytest.mark.gpu


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def H(t):
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _lean(g, **over):
    ext, tracks, mask = D(g["extrinsics"]), D(over.get("tracks", g["tracks"])), D(over.get("mask", g.get("mask")))
    return [H(x) for x in TR.triangulate_tracks_masked(ext, tracks, mask, float(g["min_tri_angle"]))]


def _batched(g, expanded_view=False):
    S, N = g["tracks"].shape[:2]
    cams = D(g["extrinsics"])[None].expand(N, -1, -1, -1)
    if not expanded_view:
        cams = cams.contiguous()                                  # real per-point cameras: the per-group kernel
    mask = None if "mask" not in g else D(g["mask"]).t()
    return [H(x) for x in TH.triangulate_multi_view_point_batched(cams, D(g["tracks"]).permute(1, 0, 2), mask,
                                                                  compute_tri_angle=True, check_cheirality=True)]


@pytest.mark.parametrize("name", MC.TRI_CASES)
def test_lean_and_namesake_equal_the_reference(name):
    g = MC.load(name)
    thr = float(g["min_tri_angle"])
    pts, valid, ang, flag = _lean(g)
    assert pts.dtype == np.float64 and ang.dtype == np.float64 and valid.dtype == np.bool_ and flag.dtype == np.bool_
    ref_max = g["ref_angles"].max(1)
    da, dc = MC.angle_deviation(ang, ref_max, g["admit_points"])
    MC.assert_close(f"lean {name}", {"points": MC.point_deviation(pts, g["ref_points"], g["admit_points"]), "angles": da,
                                     "cosines": dc})
    assert (valid == ~g["ref_invalid"])[g["admit_che"]].all()
    assert (flag == (ref_max >= thr))[g["admit_flag"]].all()
    bp, table, inv = _batched(g)
    assert table.shape == g["ref_angles"].shape
    da, dc = MC.angle_deviation(table, g["ref_angles"], g["admit_points"][:, None])
    MC.assert_close(f"batched {name}", {"points": MC.point_deviation(bp, g["ref_points"], g["admit_points"]), "angles": da,
                                        "cosines": dc})
    assert (inv == g["ref_invalid"])[g["admit_che"]].all()
    # namesake and lean form, per-point and shared cameras: the same bits
    assert same_bits(bp, pts) and same_bits(inv, ~valid) and same_bits(table.max(1), ang)
    assert (np.diagonal(table.reshape(len(table), g["tracks"].shape[0], -1), axis1=1, axis2=2) == 0).all()
    vp, vtable, vinv = _batched(g, expanded_view=True)
    assert same_bits(vp, bp) and same_bits(vtable, table) and same_bits(vinv, inv)
    # the table alone
    S, N = g["tracks"].shape[:2]
    again = H(TH.calculate_triangulation_angle_batched(D(g["extrinsics"])[None].expand(N, -1, -1, -1).contiguous(), D(bp)))
    assert same_bits(again, table)
    only = H(TR.max_triangulation_angle(D(g["extrinsics"]), D(pts)))
    assert same_bits(only, ang)


def test_from_tracks_equals_the_reference():
    g = MC.load("from_tracks")
    pts, che = (H(x) for x in TR.triangulate_multi_view_point_from_tracks(D(g["extrinsics"]), D(g["tracks"]), D(g["mask"])))
    assert pts.shape == g["ref_points"].shape and che.shape == g["ref_cheirality"].shape and che.dtype == np.bool_
    MC.assert_close("from_tracks", {"points": MC.point_deviation(pts, g["ref_points"], g["admit_points"])})
    assert (che == g["ref_cheirality"])[g["admit_che"]].all()
    lean = [H(x) for x in TR.triangulate_tracks_masked(D(g["extrinsics"][0]), D(g["tracks"][0]), D(g["mask"][0]))]
    assert same_bits(lean[0], pts[0]) and same_bits(lean[1], che[0])


@pytest.mark.parametrize("name", MC.LR_CASES)
def test_local_refinement_equals_the_reference(name):
    g = MC.load(name)
    lo, thr = int(g["lo_num"]), float(g["min_tri_angle"])
    args = (D(g["points1"]), D(g["extrinsics"]), thr, D(g["inlier_mask"]), D(g["sorted_indices"]))
    pts, flag, inv = (H(x) for x in TH.local_refinement_tri(*args, lo_num=lo))
    B, N = g["points1"].shape[:2]
    assert pts.shape == (B, lo, 3) and flag.shape == (B, lo) and inv.shape == (B, lo)
    assert pts.dtype == np.float64 and flag.dtype == np.bool_ and inv.dtype == np.bool_
    MC.assert_close(name, {"points": MC.point_deviation(pts, g["ref_points"], g["admit_points"])})
    assert (flag == g["ref_tri_angle_masks"])[g["admit_flag"]].all()
    assert (inv == g["ref_invalid"])[g["admit_che"]].all()
    other = [H(x) for x in TH.local_refinement_tri(*args, lo_num=lo, low_mem=False)]
    assert same_bits(other[0], pts) and same_bits(other[1], flag) and same_bits(other[2], inv)
    # each candidate is the namesake's solve of its own views (the observations outside them read as zero)
    lo_mask = g["inlier_mask"][np.arange(B)[:, None], g["sorted_indices"][:, :lo]]
    p = np.where(lo_mask[..., None], g["points1"][:, None], 0.0).reshape(B * lo, N, 2)
    bp, table, binv = (H(x) for x in TH.triangulate_multi_view_point_batched(
        D(np.repeat(g["extrinsics"], lo, axis=0)), D(p), D(lo_mask.reshape(B * lo, N)), compute_tri_angle=True,
        check_cheirality=True))
    assert same_bits(bp.reshape(B, lo, 3), pts) and same_bits(binv.reshape(B, lo), inv)
    assert same_bits((table >= thr).any(1).reshape(B, lo), flag)


def test_angle_functions_equal_the_reference():
    g = MC.load("angles")
    got = {"batched": H(TH.calculate_triangulation_angle_batched(D(g["batched_extrinsics"]), D(g["batched_points"]),
                                                                 float(g["batched_eps"]))),
           "exhaustive": H(TH.calculate_triangulation_angle_exhaustive(D(g["exhaustive_extrinsics"]), D(g["exhaustive_points"]))),
           "pairs": H(TH.calculate_triangulation_angle(D(g["pairs_center1"]), D(g["pairs_center2"]), D(g["pairs_points"]),
                                                       float(g["pairs_eps"])))}
    for what, a in got.items():
        ref = g[f"ref_{what}"]
        assert a.shape == ref.shape and a.dtype == np.float64
        da, dc = MC.angle_deviation(a, ref)
        MC.assert_close(f"angles {what}", {"angles": da, "cosines": dc})
        i, j = MC.EPS_BRANCH[what]
        assert a[i, j] == 0.0 and ref[i, j] == 0.0
    S = g["exhaustive_extrinsics"].shape[0]
    assert (got["exhaustive"].reshape(S, S, -1)[np.arange(S), np.arange(S)] == 0).all()
    # the exhaustive table is the batched one of the same cameras, transposed
    P = g["exhaustive_points"].shape[0]
    shared = H(TH.calculate_triangulation_angle_batched(D(g["exhaustive_extrinsics"])[None].expand(P, -1, -1, -1),
                                                        D(g["exhaustive_points"])))
    assert same_bits(shared.T, got["exhaustive"])


def test_angular_error_equals_the_reference():
    g = MC.load("angerr")
    for deg in (False, True):
        a, c = (H(x) for x in TH.calculate_normalized_angular_error_batched(D(g["point2D"]), D(g["point3D"]),
                                                                            D(g["cam_from_world"]), to_degree=deg))
        ref = g["ref_deg"] if deg else g["ref_rad"]
        assert a.shape == ref.shape == c.shape
        da, dc = MC.angle_deviation(a, ref, unit=np.pi / 180.0 if deg else 1.0, ref_cos=g["ref_cos"], got_cos=c)
        MC.assert_close(f"angerr deg={deg}", {"angles": da, "cosines": dc})
        assert c.max() <= 1.0 and c.min() >= -1.0


@pytest.mark.parametrize("name", ("bool_s8", "float_s8", "nomask_s6"))
def test_any_split_into_launches_and_any_repetition_gives_the_same_bits(name):
    g = MC.load(name)
    whole = _lean(g)
    again = _lean(g)
    assert all(same_bits(x, y) for x, y in zip(whole, again))
    N = g["tracks"].shape[1]
    for cuts in ((0, 1, 64, 65, 191, N), (0, 7, 130, N), (0, N - 1, N)):
        parts = [_lean(g, tracks=g["tracks"][:, a:b], mask=None if "mask" not in g else g["mask"][:, a:b])
                 for a, b in zip(cuts[:-1], cuts[1:])]
        for k in range(4):
            assert same_bits(np.concatenate([p[k] for p in parts]), whole[k]), (cuts, k)


def test_float32_and_float64_observations_of_the_same_values_give_the_same_bits():
    g = MC.load("f32_s8")
    assert g["tracks"].dtype == np.float32
    a, b = _lean(g), _lean(g, tracks=g["tracks"].astype(np.float64))
    assert all(same_bits(x, y) for x, y in zip(a, b))


def test_bool_mask_and_its_0_1_float_mask_give_the_same_bits():
    g = MC.load("bool_s8")
    for dtype in (np.float64, np.float32):
        a, b = _lean(g), _lean(g, mask=g["mask"].astype(dtype))
        assert all(same_bits(x, y) for x, y in zip(a, b))
    n = MC.load("nomask_s6")
    a, b = _lean(n), _lean(n, mask=np.ones(n["tracks"].shape[:2], bool))
    assert all(same_bits(x, y) for x, y in zip(a, b))


def test_float_weights_enter_squared():
    """Scaling EVERY weight by one factor leaves the points where they are (the normal matrix scales by the factor squared),
    and a weight of 2 on a view equals that view counted four times."""
    g = MC.load("float_s8")
    a = _lean(g)
    b = _lean(g, mask=g["mask"] * 2.0)                              # a power of two: the same bits
    assert same_bits(a[0], b[0])
    S, N = g["tracks"].shape[:2]
    w = np.ones((S, N))
    w[0] = 2.0
    four = dict(extrinsics=np.concatenate([g["extrinsics"], np.repeat(g["extrinsics"][:1], 3, 0)]),
                tracks=np.concatenate([g["tracks"], np.repeat(g["tracks"][:1], 3, 0)]), min_tri_angle=g["min_tri_angle"])
    x, y = _lean(g, mask=w)[0], _lean(four)[0]
    dev = np.abs(x - y).max() / np.abs(y).max()
    print(f"[multiview] weight 2 against four copies of the view: {dev:.3e}")
    assert dev <= MC.POINT_TOL


def test_points_with_fewer_than_two_weighted_views_are_nan_and_invalid():
    g = MC.load("bool_s8")
    whole = _lean(g)
    for dtype in (bool, np.float64):
        mask = g["mask"].copy()
        mask[:, 3] = False                                          # no view
        mask[:, 70] = False
        mask[5, 70] = True                                          # one view
        pts, valid, ang, flag = _lean(g, mask=mask.astype(dtype))
        for n in (3, 70):
            assert np.isnan(pts[n]).all() and not valid[n] and ang[n] == 0.0 and not flag[n]
        rest = np.ones(len(pts), bool)
        rest[[3, 70]] = False
        assert all(same_bits(x[rest], y[rest]) for x, y in zip((pts, valid, ang, flag), whole))
    # the namesakes: NaN point, invalid cheirality; local refinement: no angle flag either
    S, N = g["tracks"].shape[:2]
    cams = D(g["extrinsics"])[None].expand(N, -1, -1, -1)
    bp, inv = (H(x) for x in TH.triangulate_multi_view_point_batched(cams, D(g["tracks"]).permute(1, 0, 2), D(mask).t(),
                                                                     check_cheirality=True))
    assert np.isnan(bp[[3, 70]]).all() and inv[[3, 70]].all() and np.isfinite(bp[rest]).all()
    inl = torch.zeros(2, 3, S, dtype=torch.bool, device="cuda")
    inl[:, 0, :4] = True
    inl[:, 1, 2] = True
    idx = torch.tensor([[0, 1, 2], [2, 1, 0]], device="cuda")
    p, f, i = (H(x) for x in TH.local_refinement_tri(D(g["tracks"]).permute(1, 0, 2)[:2], cams[:2], 1.5, inl, idx, lo_num=3))
    expect_nan = np.array([[False, True, True], [True, True, False]])
    assert (np.isnan(p).all(-1) == expect_nan).all() and i[expect_nan].all() and not f[expect_nan].any()
    assert f[~expect_nan].all() and not i[~expect_nan].any()


def _torch_restatement(ext, tracks, w):
    """triangulate_multi_view_point_batched in plain torch ops on shared cameras: ext (S,3,4), tracks (S,N,2) f64, w (S,N) f64"""
    h = torch.cat([tracks, torch.ones_like(tracks[..., :1])], -1)
    r = h / h.norm(dim=-1, keepdim=True)
    terms = ext[:, None] - r[..., :, None] * torch.einsum("sni,sik->snk", r, ext)[:, :, None, :]
    terms = terms * w[:, :, None, None]
    A = torch.einsum("snij,snik->njk", terms, terms)
    v = torch.linalg.eigh(A)[1][:, :, 0]
    X = v[:, :3] / v[:, 3:]
    z = torch.einsum("sj,nj->ns", ext[:, 2, :3], X) + ext[None, :, 2, 3]
    return X, z


def test_100k_tracks_200_views_against_torch_on_the_same_device():
    S, N = 200, 100000
    rng = np.random.default_rng(7)
    ext = np.zeros((S, 3, 4))
    ext[:, :, :3] = np.eye(3)
    centres = np.stack([rng.uniform(-2, 2, S), rng.uniform(-1, 1, S), -5 + rng.uniform(-0.5, 0.5, S)], 1)
    ext[:, :, 3] = -centres
    ext_d = D(ext)
    g = torch.Generator(device="cuda").manual_seed(3)
    X = torch.rand(N, 3, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    cam = X[None] + ext_d[:, None, :, 3]
    tracks = (cam[..., :2] / cam[..., 2:] + 1e-3 * torch.randn(S, N, 2, generator=g, device="cuda", dtype=torch.float64)).float()
    keep = torch.rand(S, N, generator=g, device="cuda") < 0.5
    pts, valid, ang, flag = TR.triangulate_tracks_masked(ext_d, tracks, keep, 1.5)
    Xt, z = _torch_restatement(ext_d, tracks.double(), keep.double())
    rel = ((pts - Xt).norm(dim=1) / Xt.norm(dim=1)).max().item()
    print(f"[multiview] 100k x 200 against torch: points {rel:.3e}")
    assert rel <= MC.POINT_TOL
    clear = z.abs().min(1).values >= 1e-6
    assert bool((valid == ~(z <= 0).any(1))[clear].all()) and bool(valid.all())
    sub = torch.arange(0, N, 97, device="cuda")
    c = D(MC.np_centers(ext))
    P = pts[sub]
    sq = lambda d: d.norm(dim=-1) ** 2
    r = sq(P[:, None] - c[None])                                                    # (n,S)
    den = 2.0 * torch.sqrt(r[:, :, None] * r[:, None, :])
    nom = r[:, :, None] + r[:, None, :] - sq(c[:, None] - c[None])[None]
    th = torch.acos(torch.clamp(torch.where(den <= 1e-12, torch.ones_like(nom), nom) /
                                torch.where(den <= 1e-12, torch.ones_like(den), den), -1.0, 1.0)).abs()
    best = (torch.min(th, torch.pi - th) * (180.0 / torch.pi)).flatten(1).max(1).values
    da = (ang[sub] - best).abs().max().item()
    print(f"[multiview] 100k x 200 against torch: largest angle of {len(sub)} points {da:.3e}")
    assert da <= MC.ANGLE_TOL and bool((flag[sub] == (best >= 1.5)).all())
