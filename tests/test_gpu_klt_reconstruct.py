"""Frames in, reconstruction out, with no learned part: GeometryRunner.reconstruct_from_frames on scene A of
tests/klt_cases.py -- 8 frames of 128 x 160 rendered from 120 Gaussian blobs at projected 3D points, the camera path of
vggsfm_amd.scene scaled to an arc of 6 degrees (a blob moves 0.84 px between neighbouring frames at the most, 5.6 px in all;
at 12 degrees the blobs of different depths that share a window pull fewer than 60 % of the tracks through).  On it the
restatement of the tracker (radius 4, nms_radius 2) finds 69 corners and keeps 85.5 % of them visible in the worst frame
(frames 0 .. 7: 100, 100, 100, 97.1, 94.2, 91.3, 85.5, 85.5 %).

The yardstick is the same scene through sparse_reconstruct_from_tracks(None, ...) on the restatement's tracks, stored in
tests/golden/klt_scene_a.npz (scripts/make_golden_klt.py), under 3 seeds of the global generators; the run from frames must
stay within 2 x the largest value of each error -- the bound and the reason of tests/test_gpu_camera_prior.py.  Errors: mean
over all frame pairs of pose_pair_errors (degrees) against the ground truth carried into the estimate's world by
sim3.align_cameras, and the median distance of the points to the ground truth's (the 3D point of the blob whose centre in
the query frame is within 1.5 px of the track's query point) in ground-truth units.  Every figure is printed before it is
asserted.

Measured (one MI355X; from frames / largest of the yardstick's runs, which are identical -- the kernels' float32 tracks lead
to the same inlier sets and the same optimum as the restatement's): rotation 8.4565e-1 / 8.4565e-1 deg, translation
4.7933e+1 / 4.7933e+1 deg, median point 6.0231 / 6.0231 over 54 points.  Both are poor reconstructions: at the density the
80 % rule allows the arc is 6 degrees, and 5.6 px of parallax under tracks that are off by 0.12 px in the median and 1 px at
the 90th percentile (blobs of different depths share windows) leaves depth nearly free.  The test says that the kernels
reconstruct what the restatement reconstructs, not that either is good; extra points: 102 .. 107 per frame, largest
reprojection error 1.54 px."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import klt_cases as C
from vggsfm_amd import sim3
from vggsfm_amd.runners import GeometryConfig, GeometryRunner
from vggsfm_amd.utils.metric import pose_pair_errors

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "klt_scene_a.npz")
S = C.SCENE_A["frames"]


def D(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@functools.lru_cache(maxsize=None)
def _scene():
    sc = C.projected_scene(**C.SCENE_A)
    g = np.load(GOLDEN)
    assert all(g[f"scene_{k}"] == v for k, v in C.SCENE_A.items())
    assert np.array_equal(g["points3D"], sc["points3D"]) and np.array_equal(g["extrinsics"], sc["extrinsics"])
    return sc, g, D(sc["images"])[None]


def _errors(pred, query):
    """(rotation deg, translation deg, median point) of a predictions dict whose tracks start at `query` (N,2)"""
    sc = _scene()[0]
    ext = pred["extrinsics_opencv"].double()
    assert ext.shape == (S, 3, 4)
    (scale, R, t, ok), gt_in_est = sim3.align_cameras(D(sc["extrinsics"]), ext)
    assert bool(ok)
    rot, trans = pose_pair_errors(ext, gt_in_est)
    d = np.hypot(*(query[:, None] - sc["uv"][0][None]).transpose(2, 0, 1))
    near, known = d.argmin(1), d.min(1) < 1.5
    valid = pred["valid_tracks"].cpu().numpy().astype(bool)
    keep = known[valid]
    gt_pts = sim3.transform_points(D(sc["points3D"][near[valid]]), scale, R, t)
    point = ((pred["points3D"].double() - gt_pts).norm(dim=1) / scale)[D(keep)].median()
    return float(rot.mean()), float(trans.mean()), float(point), int(keep.sum())


@functools.lru_cache(maxsize=None)
def _yardstick():
    _, g, images = _scene()
    runs = []
    for seed in range(3):
        torch.manual_seed(seed)
        np.random.seed(seed)
        pred = GeometryRunner(GeometryConfig()).sparse_reconstruct_from_tracks(
            None, D(g["tracks"])[None], D(g["vis"])[None], D(g["score"])[None], images, back_to_original_resolution=False)
        assert pred["reconstruction"].num_reg_images() == S
        runs.append(_errors(pred, g["query"]))
    return runs


@functools.lru_cache(maxsize=None)
def _from_frames():
    images = _scene()[2]
    torch.manual_seed(0)
    np.random.seed(0)
    return GeometryRunner(GeometryConfig()).reconstruct_from_frames(images, **C.SCENE_A_TRACKER)


def test_golden_tracks_keep_80_percent_visible():
    g = _scene()[1]
    vis = g["vis"].mean(1)
    print(f"\n{g['tracks'].shape[1]} tracks, visible per frame {vis.round(3).tolist()}")
    assert g["tracks"].shape[0] == S and vis.min() >= 0.8


def test_reconstruct_from_frames_registers_all_frames_within_twice_the_yardstick():
    pred = _from_frames()
    query = pred["pred_track"][0, 0].cpu().numpy().astype(np.float64)
    mine, runs = _errors(pred, query), _yardstick()
    worst = [max(r[k] for r in runs) for k in range(3)]
    print(f"\n{len(query)} tracks from frames ({mine[3]} points compared), {_scene()[1]['tracks'].shape[1]} golden tracks "
          f"({runs[0][3]} points compared)")
    for k, what in enumerate(("rotation deg", "translation deg", "median point")):
        print(f"{what}: from frames {mine[k]:.4e}, yardstick max {worst[k]:.4e} (runs {[f'{r[k]:.4e}' for r in runs]})")
    assert pred["reconstruction"].num_reg_images() == S and pred["extrinsics_opencv"].shape == (S, 3, 4)
    assert pred["pred_vis"][0].mean(dim=1).min() >= 0.8
    for k in range(3):
        assert mine[k] <= 2.0 * worst[k]


def test_extra_tracker_through_triangulate_extra_points():
    """The tracker's callback through its consumer, pixel_interval = 8, on the refined cameras: every returned point
    reprojects into its own frame within cfg.max_reproj_error, and at least 6 of the 8 frames return a point."""
    pred = _from_frames()
    images = _scene()[2]
    cfg = GeometryConfig(extra_pt_pixel_interval=8)
    H, W = images.shape[-2:]
    boxes = torch.tensor([0.0, 0.0, W - 1.0, H - 1.0], device="cuda").expand(1, S, 4)
    paths = [f"image_{s}" for s in range(S)]
    ext, K = pred["extrinsics_opencv"], pred["intrinsics_opencv"]
    out = GeometryRunner(cfg).triangulate_extra_points(images, boxes, K, pred["extra_params"], ext, paths, S,
                                                       pred["tracker"].extra_tracker)
    counts = []
    for s, name in enumerate(paths):
        pts, uv = out[name]["points3D"].double(), out[name]["uv"].double()
        counts.append(len(pts))
        if len(pts):
            cam = pts @ ext[s, :, :3].double().T + ext[s, :, 3].double()
            proj = (cam @ K[s].double().T)
            err = (proj[:, :2] / proj[:, 2:] - uv).norm(dim=1)
            print(f"frame {s}: {len(pts)} points, largest reprojection error {float(err.max()):.3f} px")
            assert bool((cam[:, 2] > 0).all()) and float(err.max()) <= cfg.max_reproj_error
    print(f"points per frame {counts}")
    assert sum(c > 0 for c in counts) >= 6
