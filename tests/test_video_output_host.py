"""Host side of the video output tail (tests/golden/video_output_*.npz, scripts/make_golden_video_output.py): the
reference's index rule of ``_update_points_color`` restated in numpy on the procedural frames reproduces its colours, and
``VideoGeometry.dicts_to_output`` -- run on a CPU table with the golden's colours, so nothing of it needs a GPU --
assembles the reference's model and predictions."""
import glob
import hashlib
import os

import numpy as np
import pytest
import torch

from tests.video_output_frames import pixel_values
from vggsfm_amd.track_table import TrackTable
from vggsfm_amd.video import VideoGeometry

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("video_output_"):-4] for p in glob.glob(os.path.join(GOLD, "video_output_*.npz")))
COLORED = [c for c in CASES if not c.endswith("_raises")]


def load(case):
    return np.load(os.path.join(GOLD, f"video_output_{case}.npz"), allow_pickle=False)


def table_arrays(g):
    """The observation table, camera and poses of a golden case (point-major, sorted by (point, frame))."""
    if "source" in g:
        s = np.load(os.path.join(GOLD, f"{g['source']}.npz"), allow_pickle=False)
        i = int(g["source_snapshot"])
        t = dict(obs_point=s[f"s{i}_obs_point"].astype(np.int64), obs_frame=s[f"s{i}_obs_frame"].astype(np.int64),
                 obs_uv=s[f"s{i}_obs_uv"], xyz=s[f"s{i}_xyz"].astype(np.float64), extri=s[f"s{i}_extri"],
                 intrinsics=s[f"s{i}_intrinsics"], extra=s[f"s{i}_extra"])
        assert hashlib.sha256(np.ascontiguousarray(t["obs_uv"]).tobytes()).hexdigest() == str(g["table_sha256"])
        return t
    return {k: g[f"in_{k}"] for k in ("obs_point", "obs_frame", "obs_uv", "xyz", "extri", "intrinsics", "extra")}


def numpy_colors(t, seed, H, W, reverse=False):
    """video_runner.py:475-492 restated: per point the float32 mean of the pixels at (floor(v), floor(u)) (reverse:
    (floor(u), floor(v))) over the observations with floor(v) < H and floor(u) < W, negative indices from the end.
    Raises IndexError where the reference does.  Returns (rgb (P,3) float32, has (P,) bool)."""
    uv = t["obs_uv"]
    u = np.floor(uv[:, 0]).astype(np.int64)
    v = np.floor(uv[:, 1]).astype(np.int64)
    ok = (v < H) & (u < W)
    y, x = (u, v) if reverse else (v, u)
    y, x = y[ok], x[ok]
    if (y < -H).any() or (y >= H).any() or (x < -W).any() or (x >= W).any():
        raise IndexError("pixel index out of range")
    y, x = np.where(y < 0, y + H, y), np.where(x < 0, x + W, x)
    col = pixel_values(seed, t["obs_frame"][ok], y, x)
    P = len(t["xyz"])
    pt = t["obs_point"][ok]
    rgb = np.zeros((P, 3), np.float32)
    n = np.bincount(pt, minlength=P)
    for k in range(len(pt)):                                # (the table's order: ascending frame per point)
        rgb[pt[k]] += col[k]
    has = n > 0
    rgb[has] /= n[has, None].astype(np.float32)
    return rgb, has


@pytest.mark.parametrize("case", CASES)
def test_index_rule_reproduces_the_reference_colours(case):
    g = load(case)
    t = table_arrays(g)
    H, W, seed, reverse = int(g["H"]), int(g["W"]), int(g["seed"]), bool(g["reverse"])
    if bool(g["raises"]):
        with pytest.raises(IndexError):
            numpy_colors(t, seed, H, W, reverse)
        return
    rgb, has = numpy_colors(t, seed, H, W, reverse)
    assert np.array_equal(has, g["has_color"])
    np.testing.assert_allclose(rgb, g["rgb"], atol=1e-6, rtol=0)
    near = np.abs((g["rgb"].astype(np.float64) * 255) % 1.0 - 0.5) < 1e-4
    c8 = np.round(rgb * np.float32(255)).astype(np.uint8)
    mism = (c8 != g["point_color"]).any(1) & ~near.any(1)
    assert not mism.any(), np.nonzero(mism)[0][:8]
    if case != "radial_t60":                                 # the constructed cases hold every edge of the rule
        u = np.floor(t["obs_uv"][:, 0])
        assert (u < 0).any() and (u == W - 1).any() and (u == W).any() and (~has).any() and \
            (np.bincount(t["obs_point"]) == 1).any()


def cpu_geometry(g, t, colors=None):
    """A VideoGeometry on the CPU holding the golden's table; `colors`: (rgb, has) to install as update_points_color's."""
    dev = torch.device("cpu")
    cam = str(g["camera_type"])
    vg = VideoGeometry(torch.from_numpy(t["intrinsics"]).float(), torch.from_numpy(t["extra"]).float(), cam, device=dev)
    tab = TrackTable(dev)
    tab.xyz = torch.from_numpy(t["xyz"])
    tab.rgb = torch.zeros((len(t["xyz"]), 3))
    tab.obs_point = torch.from_numpy(t["obs_point"])
    tab.obs_frame = torch.from_numpy(t["obs_frame"])
    tab.obs_uv = torch.from_numpy(np.ascontiguousarray(t["obs_uv"]))
    tab.obs_vis = torch.ones(len(t["obs_point"]))
    tab.set_extrinsics(0, torch.from_numpy(t["extri"]))
    vg.table = tab
    if colors is not None:
        tab.rgb = torch.from_numpy(colors[0])
        vg.points_colored = torch.from_numpy(colors[1])
    return vg


def output_kwargs(g):
    T, H, W = int(g["T"]), int(g["H"]), int(g["W"])
    crop = torch.from_numpy(g["crop"])[None, None].expand(1, T, -1).clone()
    return dict(image_paths=[str(p) for p in g["image_paths"]], crop_params=crop, image_size=(W, H),
                back_to_original_resolution=bool(g["back"]), shift_point2d_to_original_res=bool(g["shift"]),
                shared_camera=bool(g["shared"]))


def check_output(pred, g, xyz_rtol=0.0):
    """The predictions dict against the golden's record of the reference's (tolerances of the issue's (c))."""
    rec = pred["reconstruction"]
    pids = sorted(rec.points3D)
    assert np.array_equal(pids, g["point_ids"])
    xyz = np.stack([rec.points3D[p].xyz for p in pids])
    np.testing.assert_allclose(xyz, g["point_xyz"], rtol=max(xyz_rtol, 1e-6), atol=1e-12 if xyz_rtol == 0 else xyz_rtol)
    assert np.array_equal(np.stack([rec.points3D[p].color for p in pids]), g["point_color"])
    cams = sorted(rec.cameras)
    assert np.array_equal(cams, g["camera_ids"])
    assert [rec.cameras[k].model for k in cams] == [str(m) for m in g["camera_model"]]
    assert np.array_equal([[rec.cameras[k].width, rec.cameras[k].height] for k in cams], g["camera_wh"])
    np.testing.assert_allclose(np.stack([rec.cameras[k].params for k in cams]), g["camera_params"], rtol=1e-6)
    ims = sorted(rec.images)
    assert np.array_equal(ims, g["image_ids"])
    assert [rec.images[i].name for i in ims] == [str(n) for n in g["image_names"]]
    assert np.array_equal([rec.images[i].camera_id for i in ims], g["image_camera"])
    assert all(rec.images[i].registered for i in ims) and bool(g["image_registered"].all())
    pose = np.stack([rec.images[i].cam_from_world.matrix() for i in ims])
    assert np.array_equal([len(rec.images[i].points2D) for i in ims], g["p2d_counts"])
    ids = np.concatenate([[p.point3D_id for p in rec.images[i].points2D] for i in ims]).astype(np.int64)
    xy = np.concatenate([np.array([p.xy for p in rec.images[i].points2D], np.float64).reshape(-1, 2) for i in ims])
    if "p2d_ids" in g:
        assert np.array_equal(ids, g["p2d_ids"])
        if bool(g["shift"]) and bool(g["back"]):
            np.testing.assert_allclose(xy, g["p2d_xy"], rtol=1e-12, atol=0)
        else:
            assert np.array_equal(xy, g["p2d_xy"])
    else:
        assert hashlib.sha256(ids.tobytes()).hexdigest() == str(g["p2d_ids_sha256"])
        assert hashlib.sha256(np.ascontiguousarray(xy).tobytes()).hexdigest() == str(g["p2d_xy_sha256"])
    # predictions
    ext = pred["extrinsics_opencv"].cpu().numpy()
    assert ext.dtype == np.float64 and ext.shape == g["pred_extrinsics"].shape
    np.testing.assert_allclose(pred["intrinsics_opencv"].cpu().numpy(), g["pred_intrinsics"], rtol=1e-6, atol=0)
    if "pred_extra_params" in g:
        np.testing.assert_allclose(pred["extra_params"].cpu().numpy(), g["pred_extra_params"], rtol=1e-6, atol=0)
    else:
        assert pred["extra_params"] is None
    assert pred["points3D"].dtype == torch.float32 and pred["points3D_rgb"].dtype == torch.float32
    assert tuple(pred["points3D_rgb"].shape) == g["pred_points3D_rgb"].shape
    assert all(pred[k] is None for k in ("unproj_dense_points3D", "valid_2D_mask", "pred_track", "pred_vis", "pred_score",
                                         "valid_tracks"))
    return pose, ext


@pytest.mark.parametrize("case", COLORED)
def test_model_assembly_matches_the_reference(case):
    g = load(case)
    t = table_arrays(g)
    vg = cpu_geometry(g, t, (g["rgb"], g["has_color"]))
    pred = vg.dicts_to_output(0, int(g["T"]), **output_kwargs(g))
    pose, ext = check_output(pred, g)
    assert np.array_equal(pose, g["image_pose"]) and np.array_equal(ext, g["pred_extrinsics"])
    assert np.array_equal(pred["points3D"].numpy(), g["pred_points3D"])
    assert np.array_equal(pred["points3D_rgb"].numpy(), g["pred_points3D_rgb"])


def test_output_without_colours_is_zero_and_other_ranges_are_refused():
    g = load("nonsquare_radial")
    t = table_arrays(g)
    vg = cpu_geometry(g, t)
    pred = vg.dicts_to_output(0, int(g["T"]), **output_kwargs(g))
    rec = pred["reconstruction"]
    assert all((rec.points3D[p].color == 0).all() for p in rec.points3D)
    assert float(pred["points3D_rgb"].abs().max()) == 0.0
    with pytest.raises(ValueError):
        vg.dicts_to_output(1, int(g["T"]), **output_kwargs(g))
