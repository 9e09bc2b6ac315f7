"""``geometric_camera_prior`` on the device: tracks in, reconstruction out, no learned prior.

Scenes (``vggsfm_amd.scene.make_scene``, noise 0.5 px, 5 % outliers -- the smallest at which the initial-pair rule, >= 100
inliers that are >= a quarter of the tracks, and a second registration round both occur):

    a   8 frames,  600 tracks, SIMPLE_PINHOLE, a camera per frame
    b  10 frames,  800 tracks, SIMPLE_RADIAL, one shared camera
    c   6 frames,  400 tracks, SIMPLE_PINHOLE, a camera per frame; the last frame sees two tracks only

The yardstick of the end-to-end tests is the existing path on the same tracks and the same two-view dictionary, with the
stand-in prior of the other tests (ground truth through ``perturb_for_ba``'s defaults), run under 5 seeds of the global
generators; the prior-free run must stay within 2 x the largest value of each error.  Errors: mean over all frame pairs of
``pose_pair_errors`` (rotation, translation direction; degrees) against the ground truth carried into the estimate's world by
``sim3.align_cameras``, and the median distance of the points to the ground truth's under the same alignment, in ground-truth
units.  Every figure is printed before it is asserted.

Measured (one MI355X, single runs; prior-free / largest of the 5 stand-in runs, which are identical at these sizes):
    scene a   rotation 2.321e-2 / 2.249e-2 deg, translation 1.777e-1 / 1.708e-1 deg, median point 7.60e-3 / 6.85e-3
    scene b   rotation 1.4634e-2 / 1.4634e-2 deg, translation 2.8845e-2 / 2.8845e-2 deg, median point 4.3214e-3 / 4.3214e-3
    video     largest rotation error 1.353e-4 / 1.494e-4 rad, largest centre error 7.60e-4 / 7.65e-4 (without / with the prior)
    focal     747.0 ... 755.6 over the 8 frames, truth 716.8, grid cell [647.2, 750.9] (step 103.8)
"""
import functools
import types

import numpy as np
import pytest
import torch

from vggsfm_amd import sim3
from vggsfm_amd.models import Triangulator
from vggsfm_amd.pose import focal_length_factors
from vggsfm_amd.ba_options import AbsolutePoseEstimationOptions
from vggsfm_amd.scene import make_scene, perturb_for_ba
from vggsfm_amd.two_view_geo import estimate_preliminary_cameras, geometric_camera_prior
from vggsfm_amd.utils.metric import pose_pair_errors

pytestmark = pytest.mark.gpu

W = 1024
DEV = "cuda"
SCENES = {"a": (8, 600, "SIMPLE_PINHOLE", False, 0), "b": (10, 800, "SIMPLE_RADIAL", True, 0),
          "c": (6, 400, "SIMPLE_PINHOLE", False, 0)}                                   # (S, N, camera, shared, seed)
MIN_INLIERS = 30


def D(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def _scene(name):
    S, N, cam, shared, seed = SCENES[name]
    sc = make_scene(S, N, cam, shared_camera=shared, seed=seed)
    if name == "c":
        keep = np.nonzero(sc.mask[-1])[0][:2]
        sc.mask[-1] = False
        sc.mask[-1, keep] = True
        sc.vis[-1] = sc.mask[-1].astype(np.float32)
    return sc


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(tracks, vis, score) (1,S,N,..) on the device and the two-view dictionary, computed once and never modified."""
    sc = _scene(name)
    tracks, vis, score = D(sc.tracks)[None], D(sc.vis)[None], D(sc.score)[None]
    np.random.seed(0)
    _, prelim = estimate_preliminary_cameras(tracks, vis, W, W, tracks_score=score, max_error=4.0, loopresidual=True,
                                             decompose=True)
    return tracks, vis, score, prelim


def _prior(name, seed=0, **kw):
    sc = _scene(name)
    tracks, vis, score, prelim = _inputs(name)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return geometric_camera_prior(tracks, vis, W, W, tracks_score=score, preliminary_dict=prelim, camera_type=sc.camera_type,
                                  shared_camera=sc.shared_camera, generator=gen, **kw)


# ------------------------------------------------------------------------------------------------------------ 1. registration
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_scene_supports_registration(name):
    """The precondition, on the CPU: every frame (but scene c's starved one) shares >= 30 visible tracks with the frames before
    it.  (Not marked apart from the module's gpu mark: it guards the seeds of the tests below.)"""
    sc = _scene(name)
    for f in range(1, sc.S):
        shared = int((sc.mask[f] & sc.mask[:f].any(0)).sum())
        if name == "c" and f == sc.S - 1:
            assert shared <= 2
        else:
            assert shared >= MIN_INLIERS, (name, f, shared)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_registration(name):
    sc = _scene(name)
    prior = _prior(name)
    reg = prior.registered.cpu().numpy()
    print(f"scene {name}: registered {reg.astype(int).tolist()} in {prior.rounds} rounds")
    expect = np.ones(sc.S, bool)
    if name == "c":
        expect[-1] = False
    assert np.array_equal(reg, expect)
    assert 1 <= prior.rounds <= sc.S - 2
    assert prior.extrinsics.shape == (sc.S, 3, 4) and bool(torch.isfinite(prior.extrinsics).all())
    R = prior.extrinsics[:, :, :3]
    assert float((R @ R.transpose(1, 2) - torch.eye(3, device=DEV, dtype=torch.float64)).abs().max()) < 1e-9
    if name == "c":                                                    # the starved frame keeps its two-view pose
        _, _, _, prelim = _inputs(name)
        assert torch.equal(prior.extrinsics[-1, :, :3], prelim["R_opencv"][0, -1])
        assert torch.equal(prior.extrinsics[-1, :, 3], prelim["t_opencv"][0, -1])
    else:
        assert prior.rounds >= 2                                       # (the scenes are made to need a re-triangulation)


def test_fundamental_matrices_alone_are_enough():
    """A dictionary of ``estimate_preliminary_cameras(decompose=False)``: its `fmat` is decomposed, nothing is estimated again
    (numpy's generator, which ``estimate_fundamental`` draws from, stays where it was) and the cameras are those of
    ``decompose=True``."""
    from vggsfm_amd.two_view_geo import camera_prior as CP
    from vggsfm_amd.two_view_geo.estimate_preliminary import get_default_intri
    sc = _scene("a")
    tracks, vis, score, prelim = _inputs("a")
    ext = CP.two_view_cameras(prelim["fmat"][0], tracks[0], get_default_intri(W, W, DEV, torch.float64)[2])
    assert float((ext[:, :, :3] - prelim["R_opencv"][0]).abs().max()) < 1e-9
    assert float((ext[:, :, 3] - prelim["t_opencv"][0]).abs().max()) < 1e-9
    np.random.seed(7)
    before = np.random.get_state()[1].copy()
    gen = torch.Generator(device=DEV).manual_seed(0)
    prior = geometric_camera_prior(tracks, vis, W, W, tracks_score=score, generator=gen,
                                   preliminary_dict={k: prelim[k] for k in ("fmat", "fmat_inlier_mask")})
    assert np.array_equal(np.random.get_state()[1], before)
    assert bool(prior.registered.all()) and prior.rounds == _prior("a").rounds


# ------------------------------------------------------------------------------------------------------------ 2. end to end
def _errors(sc, ext, pts, valid_tracks):
    gt = D(sc.extrinsics)
    (scale, R, t, ok), gt_in_est = sim3.align_cameras(gt, ext.double())
    assert bool(ok)
    rot, trans = pose_pair_errors(ext.double(), gt_in_est)
    gt_pts = sim3.transform_points(D(sc.points3D)[valid_tracks], scale, R, t)
    point = ((pts.double() - gt_pts).norm(dim=1) / scale).median()
    return float(rot.mean()), float(trans.mean()), float(point)


def _forward(name, cams):
    sc = _scene(name)
    tracks, vis, score, prelim = _inputs(name)
    img = types.SimpleNamespace(shape=(1, sc.S, 3, W, W))              # (only .shape is read without colours)
    out = Triangulator()(cams, tracks, vis, img, prelim, pred_score=score, shared_camera=sc.shared_camera,
                         camera_type=sc.camera_type, extract_color=False)
    ext, _, _, pts, _, rec, vframes, _, vtracks = out
    assert bool(vframes.all())
    return _errors(sc, ext, pts, vtracks), rec


@functools.lru_cache(maxsize=None)
def _yardstick(name):
    sc = _scene(name)
    ext0, K0, _, _ = perturb_for_ba(sc)
    f = D(K0[:, 0, 0] / (W / 2.0)).float()
    cams = types.SimpleNamespace(R=D(ext0[:, :, :3]).float(), T=D(ext0[:, :, 3]).float(), focal_length=torch.stack([f, f], -1))
    runs = []
    for seed in range(5):
        torch.manual_seed(seed)
        np.random.seed(seed)
        runs.append(_forward(name, cams)[0])
    return runs


@pytest.mark.parametrize("name", ["a", "b"])
def test_end_to_end_within_twice_the_stand_in_prior(name):
    """Measured: see the module docstring."""
    runs = _yardstick(name)
    worst = [max(r[k] for r in runs) for k in range(3)]
    torch.manual_seed(0)
    np.random.seed(0)
    mine, rec = _forward(name, None)
    for k, what in enumerate(("rotation deg", "translation deg", "median point")):
        print(f"scene {name} {what}: prior-free {mine[k]:.4e}, stand-in max {worst[k]:.4e} (runs {[f'{r[k]:.4e}' for r in runs]})")
    assert rec.num_reg_images() == _scene(name).S
    for k in range(3):
        assert mine[k] <= 2.0 * worst[k]


# ------------------------------------------------------------------------------------------------------------ 3. focal sweep
def test_focal_sweep():
    """Scene a seen through a focal of 0.7 x max(W, H): its tracks scaled about the principal point (exactly the image of the
    same scene under that focal, every frame).  With estimate_focal_length every registration sweeps COLMAP's grid of focal
    factors around the default focal; a registered frame's focal must be within one grid step of the truth -- the step of the
    grid cell the truth falls in, which is the resolution the sweep has."""
    sc = _scene("a")
    true_f = 0.7 * W
    c = W / 2.0
    tr = (c + (sc.tracks.astype(np.float64) - c) * (true_f / sc.intrinsics[:, 0, 0])[:, None, None]).astype(np.float32)
    tracks, vis, score = D(tr)[None], D(sc.vis)[None], D(sc.score)[None]
    np.random.seed(0)
    gen = torch.Generator(device=DEV).manual_seed(0)
    prior = geometric_camera_prior(tracks, vis, W, W, tracks_score=score, estimate_focal_length=True, generator=gen)
    grid = np.array(focal_length_factors(AbsolutePoseEstimationOptions(estimate_focal_length=True))) * W
    hi = int(np.searchsorted(grid, true_f))
    step = grid[hi] - grid[hi - 1]
    focal = prior.intrinsics[:, 0, 0].cpu().numpy()
    print(f"focal sweep: registered {prior.registered.int().tolist()}, focal {np.round(focal, 1).tolist()}, truth {true_f:.1f}, "
          f"grid cell [{grid[hi - 1]:.1f}, {grid[hi]:.1f}] (step {step:.1f})")
    assert bool(prior.registered.all())
    assert np.abs(focal - true_f).max() <= step


# ------------------------------------------------------------------------------------------------------------ 4. runner, video
def test_runner_without_cameras():
    from vggsfm_amd.runners import GeometryConfig, GeometryRunner
    sc = _scene("a")
    tracks, vis, score, _ = _inputs("a")
    images = torch.rand(1, sc.S, 3, W, W, device=DEV)
    np.random.seed(0)
    torch.manual_seed(0)
    pred = GeometryRunner(GeometryConfig()).sparse_reconstruct_from_tracks(None, tracks, vis, score, images,
                                                                           back_to_original_resolution=False)
    assert "R_opencv" in pred["preliminary_dict"]
    assert pred["reconstruction"].num_reg_images() == sc.S and pred["extrinsics_opencv"].shape == (sc.S, 3, 4)
    assert pred["points3D"].shape[0] > sc.N // 2


def _video(with_prior):
    """The sequence, the simulated tracker and the simulated predictor of tests/test_gpu_video_sequence.py, 40 frames."""
    from tests.test_gpu_video_sequence import _rodrigues, _sequence
    from vggsfm_amd import video as V
    T, N, INIT, WS = 40, 4500, 16, 8
    ext, K, extra, pts, tracks, vis = _sequence(T, N, seed=3)
    tr_all, vis_all = D(tracks), D(vis)
    rng = np.random.default_rng(9)
    gen = torch.Generator(device=DEV).manual_seed(4)

    def camera_prior(f0, f1):
        e = ext[f0:f1].copy()
        Rg, s, tg = _rodrigues(rng.normal(0, 0.5, 3)), float(rng.uniform(0.5, 2.0)), rng.normal(0, 1.0, 3)
        out = np.zeros_like(e)
        for i in range(len(e)):
            Rn = _rodrigues(rng.normal(0, 0.01, 3)) @ e[i, :, :3]
            tn = e[i, :, 3] + rng.normal(0, 0.02, 3)
            out[i, :, :3] = Rn @ Rg.T
            out[i, :, 3] = s * tn - out[i, :, :3] @ tg
        return D(out)

    def track_existing(f0, f1, uv):
        dist, idx = torch.cdist(uv.double(), tr_all[f0].double()).min(dim=1)
        assert float(dist.max()) < 1e-3
        return tr_all[f0:f1][:, idx], vis_all[f0:f1][:, idx].float()

    def track_new(f0, f1):
        cand = torch.nonzero(vis_all[f0]).squeeze(1)
        sel = cand[torch.randperm(cand.numel(), device=DEV, generator=gen)[:900]]
        v = vis_all[f0:f1][:, sel].float()
        return tr_all[f0:f1][:, sel], v, torch.ones_like(v)

    idx0 = np.nonzero(vis[:INIT].sum(0) >= 4)[0][:1500]
    pred = {"extrinsics_opencv": D(ext[:INIT]), "pred_track": tr_all[:INIT][:, idx0], "pred_vis": vis_all[:INIT][:, idx0].float(),
            "valid_2D_mask": vis_all[:INIT][:, idx0], "valid_tracks": torch.ones(len(idx0), dtype=torch.bool, device=DEV),
            "points3D": D(pts[idx0] + rng.normal(0, 0.01, (len(idx0), 3))), "points3D_rgb": None}
    vg = V.VideoGeometry(D(K[:1]), D(extra[:1]), "SIMPLE_RADIAL", max_query_pts=1200, device=DEV, generator=gen)
    vg.add_initial_window(pred, 0, INIT)
    windows = []
    move = vg.move_window
    vg.move_window = lambda *a, **k: (windows.append(move(*a, **k)), windows[-1])[1]
    table = vg.run(T, INIT, WS, camera_prior if with_prior else None, track_existing, track_new, joint_BA_interval=3)
    assert bool(table.has_extri[:T].all()) and table.extri.shape[0] == T
    assert windows and all(ok for _, _, ok in windows)                 # every window succeeds at the first attempt
    est, gt = table.extri[:T], D(ext)
    aR, aT, a_s = V.align_camera_extrinsics(est, gt)
    al = V.apply_transformation(est, aR, aT, a_s)
    Rrel = torch.bmm(al[:, :, :3], gt[:, :, :3].transpose(1, 2))
    ang = torch.acos(((Rrel.diagonal(dim1=1, dim2=2).sum(1) - 1) / 2).clamp(-1, 1))
    centre = (sim3.camera_centers(al) - sim3.camera_centers(gt)).norm(dim=1)
    return float(ang.max()), float(centre.max())


def test_video_without_predictor_or_prior():
    """Final poses (largest rotation error in rad, largest centre error, after the similarity alignment of
    tests/test_gpu_video_sequence.py) within 2 x those of the same run with the synthetic prior.  Measured: DESIGN.md s. 24."""
    with_prior = _video(True)
    without = _video(False)
    print(f"video, 40 frames: rotation {without[0]:.3e} rad (with the synthetic prior {with_prior[0]:.3e}), "
          f"centre {without[1]:.3e} (with {with_prior[1]:.3e})")
    assert without[0] <= 2.0 * with_prior[0] and without[1] <= 2.0 * with_prior[1]


# ------------------------------------------------------------------------------------------------------------ 5. poisoned memory
@pytest.mark.parametrize("pattern", [0xFF, 0x7F])
def test_prior_on_poisoned_memory(pattern):
    from tests.poison import poisoned_allocations
    sc = _scene("a")
    tracks, vis, score, prelim = _inputs("a")
    plain = _prior("a", seed=3)
    with poisoned_allocations(pattern) as st:
        copy = lambda x: torch.empty(x.shape, dtype=x.dtype, device=x.device).copy_(x)
        tr, vi, so = copy(tracks), copy(vis), copy(score)
        pre = {k: copy(v) for k, v in prelim.items()}
        gen = torch.Generator(device=DEV).manual_seed(3)
        again = geometric_camera_prior(tr, vi, W, W, tracks_score=so, preliminary_dict=pre, camera_type=sc.camera_type,
                                       shared_camera=sc.shared_camera, generator=gen)
        st.check_guards()
    assert again.rounds == plain.rounds and torch.equal(again.registered, plain.registered)
    assert torch.equal(again.extrinsics, plain.extrinsics) and torch.equal(again.intrinsics, plain.intrinsics)
