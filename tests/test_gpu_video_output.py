"""The video output tail on the device (tests/golden/video_output_*.npz, scripts/make_golden_video_output.py):
``VideoGeometry.update_points_color`` (csrc/colors.hip) and ``dicts_to_output`` against the reference's own
``_update_points_color`` / ``dicts_to_output``; chunking and host-resident frames; the loop of tests/golden/video_radial_t60
end to end; and the hand-over of the predictions to sparse depth, the reprojection video and the model writer."""
import os

import numpy as np
import pytest
import torch

from tests.test_video_output_host import COLORED, CASES, check_output, cpu_geometry, load, output_kwargs, table_arrays
from tests.video_output_frames import frames_torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def gpu_geometry(g):
    vg = cpu_geometry(g, table_arrays(g))
    dev = torch.device("cuda")
    t, vg.device = vg.table, dev
    for k in ("xyz", "rgb", "obs_point", "obs_frame", "obs_uv", "obs_vis", "extri", "has_extri"):
        setattr(t, k, getattr(t, k).to(dev))
    t.device = dev
    vg.intrinsics, vg.extra_params = vg.intrinsics.to(dev), vg.extra_params.to(dev)
    return vg


def frames_of(g):
    return frames_torch(int(g["seed"]), 0, int(g["T"]), int(g["H"]), int(g["W"]), "cuda")


def check_colors(rgb, has, g):
    """(a): float32 within 1e-6 absolute; uint8 equal except where rgb * 255 lies within 1e-4 of a .5 (counted)."""
    rgb, has = rgb.cpu().numpy(), has.cpu().numpy()
    assert np.array_equal(has, g["has_color"])
    np.testing.assert_allclose(rgb, g["rgb"], atol=1e-6, rtol=0)
    near = (np.abs((g["rgb"].astype(np.float64) * 255) % 1.0 - 0.5) < 1e-4).any(1)
    c8 = np.round(rgb * np.float32(255)).astype(np.uint8)
    differ = (c8 != g["point_color"]).any(1)
    assert not (differ & ~near).any(), np.nonzero(differ & ~near)[0][:8]
    print(f"uint8 colours: {int(differ.sum())} differ, all within 1e-4 of a .5 ({int(near.sum())} such points)")
    return int(differ.sum())


@pytest.mark.parametrize("case", COLORED)
def test_colors_match_reference(case):
    g = load(case)
    vg = gpu_geometry(g)
    rgb, has = vg.update_points_color(frames_of(g), reverse=bool(g["reverse"]))
    assert vg.table.rgb is rgb and vg.points_colored is has
    check_colors(rgb, has, g)


def test_chunks_and_host_frames_are_bit_identical():
    """(b): frame_chunk 1, 7 and T, frames in host memory (pageable and pinned) and a second run give the same bits."""
    g = load("radial_t60")
    vg = gpu_geometry(g)
    frames = frames_of(g)
    T = int(g["T"])
    ref = [a.cpu().numpy() for a in vg.update_points_color(frames[None])]
    check_colors(torch.from_numpy(ref[0]), torch.from_numpy(ref[1]), g)
    runs = [("again", frames, {})] + [(f"chunk {c}", frames, dict(frame_chunk=c)) for c in (1, 7, T)]
    for name, imgs, kw in runs:
        got = [a.cpu().numpy() for a in vg.update_points_color(imgs, **kw)]
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), name
    host = frames.cpu()
    del frames
    for kw in ({}, dict(frame_chunk=7), dict(frame_chunk=T)):
        got = [a.cpu().numpy() for a in vg.update_points_color(host, **kw)]
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), ("host", kw)
    got = [a.cpu().numpy() for a in vg.update_points_color(host.pin_memory()[None], frame_chunk=5)]
    assert all(np.array_equal(a, b) for a, b in zip(got, ref)), "pinned host"


@pytest.mark.parametrize("case", COLORED)
def test_dicts_to_output_matches_reference(case):
    g = load(case)
    vg = gpu_geometry(g)
    vg.update_points_color(frames_of(g), reverse=bool(g["reverse"]))
    pred = vg.dicts_to_output(0, int(g["T"]), **output_kwargs(g))
    pose, ext = check_output(pred, g)
    assert np.array_equal(pose, g["image_pose"]) and np.array_equal(ext, g["pred_extrinsics"])
    assert pred["extrinsics_opencv"].is_cuda and pred["points3D"].is_cuda and pred["points3D_rgb"].is_cuda
    assert np.array_equal(pred["points3D"].cpu().numpy(), g["pred_points3D"])
    np.testing.assert_allclose(pred["points3D_rgb"].cpu().numpy(), g["pred_points3D_rgb"], atol=1e-6, rtol=0)


@pytest.mark.parametrize("case", [c for c in CASES if c.endswith("_raises")])
def test_index_out_of_range_raises(case):
    g = load(case)
    vg = gpu_geometry(g)
    with pytest.raises(IndexError):
        vg.update_points_color(frames_of(g), reverse=bool(g["reverse"]))


def test_video_run_end_to_end_then_output():
    """The loop of tests/video_golden_driver.py (copied set-up) on video_radial_t60, then colours and output against
    golden 1: colours with (a)'s bars (the table is bit-exact), points / poses 1e-4 absolute, intrinsics 1e-6 relative."""
    import random

    from oracle.video_world import VideoWorld
    from vggsfm_amd import video as V

    g0 = np.load(os.path.join(GOLD, "video_radial_t60.npz"), allow_pickle=False)
    g = load("radial_t60")
    T, INIT, WS = int(g0["T"]), int(g0["init"]), int(g0["window"])
    occl = {int(k): int(v) for k, v in zip(g0["occl_calls"], g0["occl_first_bad"])}
    k1 = float(g0["k1"]) if "k1" in g0 else 0.02            # (as the driver: the golden predates the field)
    world = VideoWorld(T, int(g0["N"]), int(g0["seed"]), n_new=int(g0["n_new"]), occlusions=occl, k1=k1)
    assert world.digest() == str(g0["world_sha256"])
    dev = torch.device("cuda")
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def camera_prior(f0, f1):
        return D(world.camera_prior(f0, f1))

    def track_existing(f0, f1, uv):
        tr, vis = world.track_existing(f0, f1, uv.detach().cpu().numpy())
        return D(tr), D(vis)

    def track_new(f0, f1):
        ws = f1 - f0 - 1
        tr, vis, score = world.track_new(f0, f1, [ws // 2, ws])
        return D(tr), D(vis), D(score)

    init = world.initial_prediction(INIT)
    n0 = init["tracks"].shape[1]
    pred = {"extrinsics_opencv": D(init["extrinsics"]), "pred_track": D(init["tracks"]), "pred_vis": D(init["vis"]),
            "valid_2D_mask": D(init["mask"]), "valid_tracks": torch.ones(n0, dtype=torch.bool, device=dev),
            "points3D": D(init["points3D"]), "points3D_rgb": None}
    vg = V.VideoGeometry(D(world.K)[None], torch.full((1, 1), world.k1, dtype=torch.float64, device=dev),
                         str(g0["camera_type"]), max_query_pts=int(g0["max_query_pts"]), device=dev)
    vg.add_initial_window(pred, 0, INIT)
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    vg.run(T, INIT, WS, camera_prior, track_existing, track_new, joint_BA_interval=int(g0["joint_interval"]))
    t = vg.table
    ref = table_arrays(g)
    assert np.array_equal(t.obs_point.cpu().numpy(), ref["obs_point"])
    assert np.array_equal(t.obs_frame.cpu().numpy(), ref["obs_frame"])
    assert np.array_equal(t.obs_uv.cpu().numpy(), ref["obs_uv"])
    rgb, has = vg.update_points_color(frames_of(g))
    check_colors(rgb, has, g)
    out = vg.dicts_to_output(0, T, **output_kwargs(g))
    rec = out["reconstruction"]
    pids = sorted(rec.points3D)
    assert np.array_equal(pids, g["point_ids"])
    assert np.abs(np.stack([rec.points3D[p].xyz for p in pids]) - g["point_xyz"]).max() < 1e-4
    assert np.array_equal(np.stack([rec.points3D[p].color for p in pids]), g["point_color"])
    np.testing.assert_allclose(rec.cameras[0].params[:3], g["camera_params"][0, :3], rtol=1e-6)
    assert abs(rec.cameras[0].params[3] - g["camera_params"][0, 3]) < 1e-6
    ims = sorted(rec.images)
    assert [rec.images[i].name for i in ims] == [str(n) for n in g["image_names"]]
    assert np.abs(np.stack([rec.images[i].cam_from_world.matrix() for i in ims]) - g["image_pose"]).max() < 1e-4
    assert np.array_equal([len(rec.images[i].points2D) for i in ims], g["p2d_counts"])
    np.testing.assert_allclose(out["intrinsics_opencv"].cpu().numpy(), g["pred_intrinsics"], rtol=1e-6)
    assert np.abs(out["points3D"].cpu().numpy() - g["pred_points3D"]).max() < 1e-4


def test_output_feeds_sparse_depth_reprojection_video_and_writer(tmp_path):
    """(e): the predictions go unchanged into extract_sparse_depth_and_point_from_reconstruction ->
    make_reprojection_video, and through Reconstruction.write / read."""
    from vggsfm_amd import pycolmap_compat as pc
    from vggsfm_amd.runners import GeometryRunner

    g = load("nonsquare_radial")
    vg = gpu_geometry(g)
    T = int(g["T"])
    pred = vg.finish(frames_of(g), **{k: v for k, v in output_kwargs(g).items() if k in (
        "image_paths", "crop_params", "image_size", "shift_point2d_to_original_res", "shared_camera")},
        output_dir=str(tmp_path))
    rec = pred["reconstruction"]
    back = pc.Reconstruction(str(tmp_path / "sparse"))
    assert sorted(back.images) == sorted(rec.images) and sorted(back.points3D) == sorted(rec.points3D)
    assert all((back.points3D[p].color == rec.points3D[p].color).all() for p in rec.points3D)
    runner = GeometryRunner()
    pred = runner.extract_sparse_depth_and_point_from_reconstruction(pred)
    names = [rec.images[i].name for i in sorted(rec.images)]
    assert set(pred["sparse_depth"]) <= set(names)
    w, h = int(g["crop"][0]), int(g["crop"][1])
    rng = np.random.default_rng(0)
    originals = {n: rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for n in names}
    frames = runner.make_reprojection_video(pred, (w, h), [f"/data/{n}" for n in names], originals)
    assert len(frames) == T and all(f.shape == (h, w, 3) and f.dtype == np.uint8 for f in frames)
