"""The covariance entries on the GPU (include/vggsfm_amd_covariance.h) against the long-double references of
tests/covariance_cases.py (checked by themselves in tests/test_covariance_reference.py).

vggc_spd_inverse: seeded SPD matrices (covariance_cases.spd_matrix: orthogonal factor of a Gaussian matrix, eigenvalues
1 .. 1e4, rows and columns scaled by up to 30 -- condition ~5e5) for n below, at and above one 64-block and on both sides of
128; the strict upper triangle of the input holds NaN (only the lower one may be read).  Measures: |delta_ij| / sqrt(X_ii X_jj)
with the reference's diagonal, bound max(1e-11, 100 x the float64 CPU evaluation's deviation); max |A X - I| in float64, bound
100 x what the float64 CPU inverse leaves; bitwise symmetry; two runs bit-identical.

vggc_ba_covariance (through vggsfm_amd.ba.estimate_covariance) at the perturbed start point of ten cases of
tests/ba_system_cases.py: per block type |delta_ij| / sqrt(Sigma_ii Sigma_jj), bound max(1e-11, 100 x the float64 deviation of the
case); inactive rows, columns and points exactly zero; the state bit-identical before and after; a solve afterwards equal to
the solve of a freshly compiled problem, bit for bit.

Measured on an MI355X (GPU deviation / float64 CPU deviation / bound).  vggc_spd_inverse: 2.0e-16 at n = 1, 7.5e-14 .. 2.0e-13
for n = 14 .. 200 against bounds of 1.0e-11 .. 1.8e-11, 4.2e-13 / 2.0e-13 / 2.0e-11 at n = 770; |A X - I| 8.4e-13 .. 2.8e-12
against 1.1e-10 .. 2.9e-10.  vggc_ba_covariance, pose blocks (the points' follow them; intrinsics are one to two decades
smaller):
  a 2.1e-09 / 1.3e-09 / 1.3e-07   c 2.2e-11 / 2.0e-09 / 2.0e-07   d 5.7e-10 / 2.2e-09 / 2.2e-07   e 6.0e-11 / 2.3e-09 / 2.3e-07
  h 2.4e-10 / 7.6e-09 / 7.6e-07   i_none 5.6e-11 / 1.3e-11 / 1.3e-09   i_extra 2.1e-10 / 4.1e-10 / 4.1e-08
  j 3.3e-14 / 9.8e-14 / 1.0e-11   g 1.6e-10 / 2.8e-08 / 2.8e-06
  l_env 2.1e-07 / 2.2e-05 / 2.2e-03
The device inverts the Jacobi-scaled system, whose condition is the better one: it is mostly nearer to the long-double
reference than the float64 CPU evaluation of the unscaled formulas; i_none, at 4 x that evaluation, comes closest to its bound."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ba_system_cases as SC
from tests import covariance_cases as CC
from vggsfm_amd import _lib
from vggsfm_amd import ba as BA
from vggsfm_amd.ba_options import BundleAdjustmentOptions
from vggsfm_amd.scene import make_scene, perturb_for_ba

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ vggc_spd_inverse
def spd_inverse(A_host, poison_upper=True):
    """vggc_spd_inverse on a copy of the lower triangle of `A_host`; the strict upper triangle holds NaN on entry.
    -> (inverse (n,n) numpy, failure flag)."""
    L = _lib.lib()
    n = A_host.shape[0]
    A = torch.empty((n, n), dtype=torch.float64, device="cuda")
    src = torch.from_numpy(np.ascontiguousarray(A_host)).cuda()
    if poison_upper:
        src = torch.where(torch.ones(n, n, device="cuda").tril().bool(), src, torch.full_like(src, float("nan")))
    A.copy_(src)
    ws = torch.empty(L.vggc_spd_inverse_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    fail = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(L.vggc_spd_inverse(A, n, ws, fail, _lib.stream_ptr()), "vggc_spd_inverse")
    return A.cpu().numpy(), int(fail.cpu()[0])


@pytest.mark.parametrize("n", CC.SPD_SIZES)
def test_spd_inverse_matches_the_long_double_inverse(n):
    A, ref, dev, bound, res_bound = CC.spd_reference(n)
    X, fail = spd_inverse(A)
    again, _ = spd_inverse(A)
    assert fail == 0 and np.isfinite(X).all()
    d = np.diag(ref).astype(np.float64)
    err = float((np.abs((X - ref).astype(np.float64)) / np.sqrt(np.outer(d, d))).max())
    res = float(np.abs(A @ X - np.eye(n)).max())
    print(f"\nn = {n}: GPU {err:9.2e}   float64 CPU {dev:9.2e}   bound {bound:9.2e};   |A X - I| {res:9.2e}   bound {res_bound:9.2e}")
    assert X.tobytes() == X.T.copy().tobytes(), "not bitwise symmetric"
    assert X.tobytes() == again.tobytes(), "two runs differ"
    assert err <= bound and res <= res_bound


# ------------------------------------------------------------------ vggc_ba_covariance
def _state(prob):
    return tuple(t.cpu().numpy().copy() for t in (prob.cam_q, prob.cam_t, prob.intr, prob.pts))


def _in_problem_order(prob, cov):
    """The result's per-camera blocks back in the problem's camera order (the reference's)."""
    perm = prob.cam_perm
    take = (lambda t: t) if perm is None else (lambda t: t[perm])
    n = lambda t: None if t is None else t.cpu().numpy()
    NI = prob.intr.shape[0]
    return CC.SimpleNamespace(pose=n(take(cov.pose)), intrinsics=n(take(cov.intrinsics) if NI > 1 else cov.intrinsics),
                              pose_intrinsics=n(take(cov.pose_intrinsics)) if cov.pose_intrinsics is not None else None,
                              points=n(cov.points))


@pytest.mark.parametrize("name", CC.CASES)
def test_ba_covariance_matches_the_reference(name):
    case = SC.CASES[name]
    opt = SC.options_of(case)
    prob = SC.compile_case(name, "cuda")
    SC.check_edges(name, prob)
    R = CC.reference(name, SC.host_arrays(prob, case))
    ref, pb = R.ref, R.pb
    C, NI, kd, n = pb.C, pb.NI, pb.kd, pb.n_red
    before = _state(prob)
    cov = BA.estimate_covariance(prob, opt, points=True, reduced=True)
    after = _state(prob)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after)), "the state was written"
    got = _in_problem_order(prob, cov)
    if kd == 0:
        assert cov.intrinsics is None and cov.pose_intrinsics is None
        got.intrinsics, got.pose_intrinsics = np.zeros((NI, 0, 0)), np.zeros((C, 6, 0))
    print(f"\n{name}: n = {n}, {pb.P} points, {len(pb.obs_cam)} observations, {int((~pb.active[:n]).sum())} inactive columns")
    over = {}
    for k, (err, zeros) in CC.errors(got, ref).items():
        print(f"  {k:16s} GPU {err:9.2e}   float64 CPU {R.dev[k]:9.2e}   bound {R.bounds[k]:9.2e}" + ("   EXCEEDED" if not err <= R.bounds[k] else ""))
        assert zeros, f"{k}: an inactive entry is not exactly zero"
        if not err <= R.bounds[k]:
            over[k] = (err, R.bounds[k])
    # the reduced covariance: both triangles, bitwise symmetric, the blocks are cuts of it, inactive rows and columns zero
    red = cov.reduced.cpu().numpy()
    assert red.shape == (n, n) and red.tobytes() == red.T.copy().tobytes()
    act = pb.active[:n]
    assert (red[~act] == 0).all() and (red[:, ~act] == 0).all() and (np.diag(red)[act] > 0).all()
    d = np.diag(ref.reduced).astype(np.float64)
    s = np.sqrt(np.where(act, d, 1.0))
    err = float((np.abs((red - ref.reduced).astype(np.float64)) / np.outer(s, s))[np.ix_(act, act)].max())
    print(f"  {'reduced':16s} GPU {err:9.2e}   bound {max(R.bounds.values()):9.2e}")
    assert err <= max(R.bounds.values())
    for c in (0, C // 2, C - 1):
        assert (got.pose[c] == red[6 * c:6 * c + 6, 6 * c:6 * c + 6]).all()
        if kd:
            a = 0 if NI == 1 else c
            assert (got.pose_intrinsics[c] == red[6 * c:6 * c + 6, 6 * C + kd * a:6 * C + kd * (a + 1)]).all()
            assert (got.intrinsics[a] == red[6 * C + kd * a:6 * C + kd * (a + 1), 6 * C + kd * a:6 * C + kd * (a + 1)]).all()
    # the labels of the rows and the counts
    assert len(cov.columns) == n and cov.num_active == int(pb.active.sum())
    if prob.cam_perm is not None:
        perm = prob.cam_perm.tolist()
        assert [c[1] for c in cov.columns[:6 * C:6]] == perm and (cov.pose[perm[5]].cpu().numpy() == got.pose[5]).all()
    vf = 2.0 * R.cost / (2 * len(pb.obs_cam) - int(pb.active.sum()))
    assert abs(cov.variance_factor - vf) <= 1e-12 * vf and abs(cov.cost - R.cost) <= 1e-12 * R.cost
    # poses alone: the same bits, nothing else computed
    only = BA.estimate_covariance(prob, opt, intrinsics=False)
    assert only.points is None and only.reduced is None and only.intrinsics is None and only.pose_intrinsics is None
    assert torch.equal(only.pose, cov.pose)
    assert not over, over
    # a solve afterwards is the solve of a fresh problem
    fresh = SC.compile_case(name, "cuda")
    s_fresh, _ = BA.solve(fresh, opt)
    s_here, _ = BA.solve(prob, opt)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(_state(fresh), _state(prob)))
    assert s_fresh["iterations"] == s_here["iterations"] and s_fresh["termination"] == s_here["termination"]


# ------------------------------------------------------------------ bundle_adjustment(return_covariance=True)
def test_bundle_adjustment_returns_the_covariance_of_its_solution(monkeypatch):
    sc = make_scene(8, 400, "SIMPLE_RADIAL", shared_camera=True, seed=1)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=1)
    T = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    opt = BundleAdjustmentOptions()
    opt.solver_options.max_num_iterations = 6
    args = lambda: (T(pts0), T(ext0), T(K0), T(sc.tracks), T(sc.mask), None, T(extra0), True, "SIMPLE_RADIAL", opt)
    plain = BA.bundle_adjustment(*args())
    assert "covariance" not in plain[4]
    solved = []
    inner = BA.solve

    def spy(problem, options=None, workspace=None):
        solved.append(problem)
        return inner(problem, options, workspace)
    monkeypatch.setattr(BA, "solve", spy)
    with_cov = BA.bundle_adjustment(*args(), return_covariance=True)
    for a, b in zip(plain[:4], with_cov[:4]):
        assert torch.equal(a, b)
    assert plain[4]["iterations"] == with_cov[4]["iterations"]
    cov = with_cov[4]["covariance"]
    prob = solved[0]
    direct = BA.estimate_covariance(prob, opt, points=True)
    assert torch.equal(cov.pose, direct.pose) and torch.equal(cov.intrinsics, direct.intrinsics)
    assert torch.equal(cov.pose_intrinsics, direct.pose_intrinsics)
    # points: indexed like points3D_opt (the valid tracks, ascending), the problem numbers them by track length
    valid_idx, deleted = with_cov[4]["valid_idx"], with_cov[4]["deleted"]
    assert cov.points.shape == (with_cov[0].shape[0], 3, 3) and bool((valid_idx[1:] > valid_idx[:-1]).all())
    length = torch.from_numpy(sc.mask).cuda().sum(0)
    order = valid_idx[torch.argsort(length[valid_idx], stable=True)]          # the problem's point p is input track order[p]
    back = torch.argsort(order)
    assert torch.equal(cov.points, direct.points[back])
    assert bool((cov.points[deleted] == 0).all())
    alive = ~deleted
    assert bool((torch.diagonal(cov.points[alive], dim1=1, dim2=2) > 0).all())
    assert bool((cov.pose[0] == 0).all()) and float(cov.pose[1][3, 3]) == 0.0 and float(cov.pose[2][3, 3]) > 0
    assert cov.variance_factor > 0 and cov.num_active == 6 * 8 - 7 + 2 + 3 * int(alive.sum())


def test_pycolmap_surface_uses_the_gauge_of_the_solve():
    from tests.test_pycolmap_compat import _api_build
    from vggsfm_amd import pycolmap_compat as pc
    sc = make_scene(9, 260, "SIMPLE_RADIAL", shared_camera=True, seed=11, outlier_frac=0.0)
    ext0, K0, xp0, pts0 = perturb_for_ba(sc, seed=11)
    rec = _api_build(pts0, ext0, K0, sc.tracks, sc.mask, [1024, 1024], True, "SIMPLE_RADIAL", xp0)
    xyz = rec._xyz[:rec._n].copy()
    out = pc.estimate_ba_covariance(rec)
    assert (rec._xyz[:rec._n] == xyz).all()                                  # the reconstruction is not changed
    ids = rec.reg_image_ids()
    assert sorted(out["poses"]) == sorted(ids) and all(v.shape == (6, 6) for v in out["poses"].values())
    assert (out["poses"][ids[0]] == 0).all() and out["poses"][ids[1]][3, 3] == 0 and out["poses"][ids[1]][4, 4] > 0
    assert set(out["points"]) <= set(rec.point3D_ids()) and len(out["points"]) > 200
    assert all(np.diag(v).min() > 0 for v in out["points"].values()) and out["variance_factor"] > 0
    # a config: first pose constant (all of it), the first 100 points constant, intrinsics not refined
    o = pc.BundleAdjustmentOptions()
    o.refine_focal_length = o.refine_extra_params = False
    cfg = pc.BundleAdjustmentConfig()
    for i in ids:
        cfg.add_image(i)
    cfg.set_constant_cam_pose(ids[0])
    for p in rec.point3D_ids():
        (cfg.add_constant_point if p < 101 else cfg.add_variable_point)(p)
    out2 = pc.estimate_ba_covariance(rec, o, cfg)
    assert (out2["poses"][ids[0]] == 0).all() and out2["poses"][ids[1]][3, 3] > 0     # no t_x gauge in a config
    assert all((out2["points"][p] == 0).all() for p in range(1, 101) if p in out2["points"])
    assert all(np.diag(out2["points"][p]).min() > 0 for p in out2["points"] if p >= 101)
