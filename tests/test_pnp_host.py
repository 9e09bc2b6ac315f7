"""EPnP and the local optimisation of the P3P RANSAC, the part that needs no GPU: argument validation before any launch, the CPU
yardstick of tests/pnp_cases.py checked by itself against the golden file made from the reference's own ``efficient_pnp`` (and the golden file against the
reference where its tree exists), the restated LO loop on the LO scene, and the opt-in switch."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import ref_harness
from tests import pnp_cases as PC
from vggsfm_amd import _lib, ba_options, pose
from vggsfm_amd import two_view_geo as TV
from vggsfm_amd.two_view_geo import perspective_n_points as PN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_refuse_bad_sizes_before_any_launch():
    L = _lib.lib()
    one = torch.zeros(64, dtype=torch.float64)          # (host memory: nothing is launched on these paths)
    bad, unsupported = -1, -4
    out = (one, one, one, one, one, one, one)
    assert L.vggp_epnp_solve(one, 0, one, None, 1, 3, 0, *out, None) == bad                 # fewer than four points
    assert L.vggp_epnp_solve(one, 0, one, None, -1, 8, 0, *out, None) == bad
    assert L.vggp_epnp_solve(None, 0, one, None, 1, 8, 0, *out, None) == bad
    assert L.vggp_epnp_solve(one, 0, one, None, 1, 8, 0, one, one, one, one, one, one, None, None) == bad
    assert L.vggp_epnp_solve(None, 0, None, None, 0, 8, 0, *([None] * 7), None) == 0          # no problems: a no-op
    assert L.vggp_epnp_solve(one, 0, one, None, 2 ** 31, 8, 0, *out, None) == unsupported
    assert L.vggp_pose_score(one, one, one, None, one, 1, 0, 8, one, one, None, None) == bad
    assert L.vggp_pose_score(one, one, one, None, one, 1, 2, 0, one, one, None, None) == bad
    assert L.vggp_pose_score(one, one, one, None, None, 1, 2, 8, one, one, None, None) == bad   # no thresholds
    assert L.vggp_pose_score(None, None, None, None, None, 0, 2, 8, None, None, None, None) == 0
    assert L.vggp_pose_score(one, one, one, None, one, 2 ** 30, 4, 8, one, one, None, None) == unsupported
    assert L.vggp_epnp_lo(one, one, None, one, 1, 3, 10, one, one, one, one, None) == bad
    assert L.vggp_epnp_lo(one, one, None, one, 1, 8, -1, one, one, one, one, None) == bad
    assert L.vggp_epnp_lo(one, one, None, one, 1, 8, 10, one, one, one, None, None) == bad
    assert L.vggp_epnp_lo(None, None, None, None, 0, 8, 10, None, None, None, None, None) == 0
    assert L.vggp_epnp_lo(one, one, None, one, 2 ** 31, 8, 10, one, one, one, one, None) == unsupported
    with pytest.raises(ctypes.ArgumentError):
        L.vggp_epnp_solve(one, 0, one, None, 1, 2 ** 31, 0, *out, None)


# --- the public functions -------------------------------------------------------------------------------------------------
def test_exports_and_arguments_are_validated_before_the_library_is_touched(monkeypatch):
    assert TV.efficient_pnp is PN.efficient_pnp and TV.EpnpSolution is PN.EpnpSolution
    assert PN.EpnpSolution._fields == ("x_cam", "R", "T", "err_2d", "err_3d")

    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "lib", no_library)
    x, y = torch.zeros(2, 8, 3, dtype=torch.float64), torch.zeros(2, 8, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="at least 4"):
        PN.efficient_pnp(x[:, :3], y[:, :3])
    with pytest.raises(ValueError):
        PN.efficient_pnp(x[:, :7], y)
    with pytest.raises(ValueError, match="masks"):
        PN.efficient_pnp(x, y, masks=torch.ones(2, 7))
    with pytest.raises(RuntimeError, match="no CPU path"):
        PN.efficient_pnp(x, y, masks=torch.ones(2, 8))
    P, thr = torch.zeros(2, 3, 3, 4, dtype=torch.float64), torch.ones(2, dtype=torch.float64)
    with pytest.raises(ValueError, match="poses"):
        pose.pose_score(P[:, :, :2], y, x[0], None, thr)
    with pytest.raises(ValueError, match="max_error_sq"):
        pose.pose_score(P, y, x[0], None, thr[:1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        pose.pose_score(P, y, x[0], None, thr)
    num, inl = torch.ones(2, dtype=torch.int32), torch.ones(2, 8, dtype=torch.bool)
    with pytest.raises(ValueError, match="max_rounds"):
        pose.epnp_local_optimisation(P[:, 0], num, thr, inl, y, x[0], None, thr, max_rounds=-1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pose.epnp_local_optimisation(P[:, 0], num, thr, inl, y, x[0], None, thr)


# --- the yardstick by itself ----------------------------------------------------------------------------------------------
def _differences(k, R, T, x_cam, err_2d, keep):
    return (np.linalg.norm(k["R"] - R), np.linalg.norm(k["T"] - T) / np.linalg.norm(T),
            np.linalg.norm((k["x_cam"] - x_cam)[keep]) / np.linalg.norm(x_cam[keep]), abs(k["err_2d"] - err_2d) / max(err_2d, PC.ERR_SCALE))


def test_golden_file_holds_the_cases():
    g = PC.load_golden()
    assert list(g) == list(PC.GOLDEN_CASES) and os.path.getsize(PC.GOLDEN) < 1_000_000
    for name, (n, noise, what) in PC.GOLDEN_CASES.items():
        c = g[name]
        assert c["x"].shape == (PC.GOLDEN_B, n, 3) and c["y"].shape == (PC.GOLDEN_B, n, 2) and c["x"].dtype == np.float64
        assert c["ref_R"].shape == (PC.GOLDEN_B, 3, 3) and c["ref_x_cam"].shape == c["x"].shape
        assert c["ref_kernel"].shape == (PC.GOLDEN_B, 12, 4) and c["skip"] == (what == "skip")
        if what == "six":
            assert (c["masks"].sum(1) == 6).all() and (c["x"][~c["masks"]] == 7.0).all()
        if what == "half":
            assert (c["masks"].sum(1) == n // 2).all()


@pytest.mark.parametrize("name", list(PC.GOLDEN_CASES))
def test_cpu_solver_reproduces_the_reference(name):
    """R, T, x_cam, err_2d of the CPU solver's winner against the reference's own function, with the kernel vectors signed
    as the reference's eigensolver signed them (tests/pnp_cases.py epnp: case 3 depends on those signs).  The reference
    returns no winner index: equal R and T say that the same candidate won."""
    c = PC.load_golden()[name]
    worst = np.zeros(4)
    for b in range(PC.GOLDEN_B):
        m = None if c["masks"] is None else c["masks"][b]
        cands, best = PC.epnp(c["x"][b], c["y"][b], m, c["skip"], kernel_like=c["ref_kernel"][b])
        keep = np.ones(len(c["x"][b]), bool) if m is None else m
        worst = np.maximum(worst, _differences(cands[best], c["ref_R"][b], c["ref_T"][b], c["ref_x_cam"][b], c["ref_err_2d"][b], keep))
    print(f"{name}: CPU solver against the reference: R {worst[0]:.2e}, T {worst[1]:.2e}, x_cam {worst[2]:.2e}, err_2d {worst[3]:.2e}")
    assert worst.max() <= PC.YARDSTICK_BOUND


@pytest.mark.parametrize("name", PC.NOISE_FREE)
def test_cpu_solver_recovers_the_true_pose(name):
    c = PC.load_golden()[name]
    worst = np.zeros(2)
    for b in range(PC.GOLDEN_B):
        cands, best = PC.epnp(c["x"][b], c["y"][b], None if c["masks"] is None else c["masks"][b], c["skip"])
        k = cands[best]
        worst = np.maximum(worst, (np.linalg.norm(k["R"] - c["R_true"][b]),
                                   np.linalg.norm(k["T"] - c["T_true"][b]) / np.linalg.norm(c["T_true"][b])))
    print(f"{name}: CPU solver against the true pose: R {worst[0]:.2e}, T {worst[1]:.2e}")
    assert worst.max() <= PC.TRUE_POSE_BOUND


@pytest.mark.skipif(not ref_harness.available(), reason="the reference tree is not available")
def test_golden_file_is_what_the_reference_gives():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_pnp", os.path.join(ROOT, "scripts", "make_golden_pnp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh, stored = mod.make(), np.load(PC.GOLDEN)
    assert sorted(fresh) == sorted(stored.files)
    for k in stored.files:
        assert np.array_equal(np.asarray(fresh[k]), stored[k]), k


# --- the LO restatement ---------------------------------------------------------------------------------------------------
def test_lo_restatement_on_the_lo_scene():
    sc = PC.lo_scene()
    F, P = sc["cand"].shape
    assert (F, P) == (3, 300) and sc["outlier"].sum(1).tolist() == [90, 90, 90] and not sc["cand"][2, ::3].any()
    thr = np.sqrt(sc["thr_sq"][0])
    for f in range(F):                                   # outliers are more than twenty thresholds away from the truth
        r, _ = PC.residuals(sc["pose_true"][f], sc["xn"][f], sc["X"])
        assert np.sqrt(r[sc["outlier"][f]]).min() > 20 * thr and np.sqrt(r[~sc["outlier"][f]]).max() < thr
    poses, nums = PC.p3p_incoming_cpu(sc, PC.p3p_seed_poses(sc))
    left_out = 0
    for f in range(F):
        assert nums[f] >= PC.LO_MIN_INLIERS
        pose_f, cnt, rs, mask, hist = PC.local_optimisation(poses[f], nums[f], sc["xn"][f], sc["X"], sc["cand"][f],
                                                          sc["thr_sq"][f], 10)
        print(f"frame {f}: support per round {[(c, float(f'{s:.6g}')) for c, s in hist]}; true inliers among the candidates "
              f"{int((~sc['outlier'][f] & sc['cand'][f]).sum())}")
        assert hist[0][0] == nums[f]                      # round 0 recounts what the RANSAC counted
        for (c0, s0), (c1, s1) in zip(hist, hist[1:]):   # the support never decreases
            assert c1 > c0 or (c1 == c0 and s1 < s0)
        assert cnt == mask.sum() == hist[-1][0] and len(hist) > 1
        left_out += int(PC.near_threshold(pose_f, sc["xn"][f], sc["X"], sc["cand"][f], sc["thr_sq"][f]).sum())
    print(f"matches within 1e-9 relative of their threshold under the final poses: {left_out}")
    assert left_out == 0                                  # (the cap would be 1 %: the GPU comparison leaves out nothing)


def test_lo_restatement_leaves_small_and_empty_frames_alone():
    sc = PC.lo_scene()
    pose0 = sc["pose_true"][0]
    cand = np.zeros(300, bool)
    cand[np.nonzero(~sc["outlier"][0])[0][:5]] = True     # five inliers: below the smallest set EPnP is given
    p, cnt, rs, mask, hist = PC.local_optimisation(pose0, 5, sc["xn"][0], sc["X"], cand, sc["thr_sq"][0], 10)
    assert cnt == 5 and len(hist) == 1 and p is pose0
    p, cnt, rs, mask, hist = PC.local_optimisation(np.zeros((3, 4)), 0, sc["xn"][0], sc["X"], cand, sc["thr_sq"][0], 10)
    assert cnt == 0 and hist == [] and not p.any()


# --- the switch ---------------------------------------------------------------------------------------------------------------
def test_local_optimisation_is_off_by_default_and_then_not_reached(monkeypatch):
    assert ba_options.RANSACOptions().lo_max_rounds == 0
    assert ba_options.AbsolutePoseEstimationOptions().ransac.lo_max_rounds == 0
    S, P = 2, 12
    calls = []

    def p3p_stub(xn, X, cand, samples, thr, G=1):
        calls.append("p3p")
        F = xn.shape[0]
        eye = torch.eye(3, 4, dtype=torch.float64).expand(F, 3, 4).clone()
        return (eye, torch.full((F,), P, dtype=torch.int32), torch.zeros(F, dtype=torch.float64),
                torch.zeros(F, dtype=torch.int32), torch.ones((F, P), dtype=torch.bool))

    def lo_raises(*a, **k):
        raise AssertionError("the local optimisation was reached with lo_max_rounds = 0")

    def lo_records(pose_, num, rsum, inl, *a):
        calls.append(("lo", a[-1]))
        return pose_, num, rsum, inl
    import vggsfm_amd.utils.triangulation_helpers as H
    monkeypatch.setattr(_lib, "require_gpu", lambda *a: None)
    monkeypatch.setattr(pose, "p3p_ransac", p3p_stub)
    monkeypatch.setattr(pose, "pose_refinement_batch", lambda ext, intr, *a, **k: (ext, intr, []))
    monkeypatch.setattr(H, "cam_from_img", lambda pts, K, extra: pts)
    args = (torch.eye(3, 4, dtype=torch.float64).expand(S, 3, 4), torch.ones(S, 4, dtype=torch.float64),
            torch.zeros(S, P, 2, dtype=torch.float64), torch.zeros(P, 3, dtype=torch.float64), torch.ones(S, P, dtype=torch.bool),
            [0, 1], "SIMPLE_PINHOLE", torch.zeros(S, dtype=torch.uint8))
    monkeypatch.setattr(pose, "epnp_local_optimisation", lo_raises)
    ext, intr, success, num, inl = pose.absolute_pose_estimation_batch(*args)
    assert calls == ["p3p"] and success.all() and (num == P).all()
    monkeypatch.setattr(pose, "epnp_local_optimisation", lo_records)
    opts = ba_options.AbsolutePoseEstimationOptions()
    opts.ransac.lo_max_rounds = 10
    pose.absolute_pose_estimation_batch(*args, estoptions=opts)
    assert calls == ["p3p", "p3p", ("lo", 10)]
