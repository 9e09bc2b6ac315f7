"""Frames and a sparse reconstruction in, ONE fused point cloud out, with no learned part:
GeometryRunner.dense_reconstruct_from_frames, then GeometryRunner.fuse_dense_point_cloud, on the reconstruction of
tests/test_gpu_mvs_reconstruct.py -- 6 frames of 48 x 64 under one SIMPLE_RADIAL camera (k = 0.08) in front of the slanted
plane of tests/mvs_cases.py, 24 planes, every other option at its default (4 sources, min_views 2, 1 %, 1 px, 30 degrees).

The fused cloud must equal, bit for bit, the NumPy restatement of tests/fusion_cases.py applied to the depth maps, frames
and ray maps read back from the device: no tolerance and no CPU stereo.  The distance of the points from the true plane is
that of the sweep's depth maps (their fronto-parallel bias on a plane seen at up to 29 degrees), not
of the fusion; it is asserted at 2 x what the restatement measures on the same maps, computed on the CPU in this test.

Measured (one MI355X): identical bits; 4440 points of 10155 pixels with depth (0.437), per view 1167 / 599 / 487 / 812 / 523 /
852, num_views 2 / 3 / 4 / 5: 940 / 1875 / 989 / 636; distance to the plane 1.81e-2 in the median, 0.236 at most, on both
sides (bounds 3.63e-2 and 0.472); the normals of these stereo maps are 10.2 degrees off the plane's in the median."""
import functools

import numpy as np
import pytest
import torch

from tests import fusion_cases as C
from tests import mvs_cases as MC
from vggsfm_amd import dense_depth as DD
from vggsfm_amd import fusion, mvs
from vggsfm_amd.runners import GeometryConfig, GeometryRunner
from vggsfm_amd.utils.tensor_to_pycolmap import batch_matrix_to_pycolmap

pytestmark = pytest.mark.gpu

PLANES = 24


@functools.lru_cache(maxsize=None)
def _run(tmp):
    sc = MC.reconstruction_scene()
    S, H, W = sc["frames"].shape
    K = np.zeros((S, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = sc["cams"][:, 0]
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = sc["cams"][:, 1], sc["cams"][:, 2], 1.0
    rec = batch_matrix_to_pycolmap(sc["points3D"], sc["poses"], K, sc["tracks"], sc["masks"], np.array([W, H]),
                                   shared_camera=True, camera_type="SIMPLE_RADIAL", extra_params=sc["cams"][:, 3:4])
    assert rec.num_reg_images() == S
    images = torch.from_numpy(C.colours(sc["frames"])).cuda()[None].contiguous()             # (1,S,3,H,W) colours
    runner = GeometryRunner(GeometryConfig())
    pred = runner.dense_reconstruct_from_frames({"reconstruction": rec}, images, num_planes=PLANES)
    before = {k: v for k, v in pred.items()}
    path = str(tmp / "fused.ply")
    pred = runner.fuse_dense_point_cloud(pred, images, output_path=path)
    return sc, rec, images, pred, before, path


@functools.lru_cache(maxsize=None)
def _restated(tmp):
    """the restatement on what the device holds: depth maps, frames and ray maps read back"""
    sc, rec, images, pred, _, _ = _run(tmp)
    ids = sorted(int(i) for i in rec.reg_image_ids())
    H, W = sc["frames"].shape[1:]
    depth = np.stack([pred["depth_dict"][rec.images[i].name].cpu().numpy() for i in ids])
    pose, cam = DD._camera_rows(rec, ids)
    rays, ray_index = mvs.camera_rays(cam, H, W)
    rays, ray_index = rays.cpu().numpy(), ray_index.numpy()
    chosen = mvs.select_source_views(rec, 4)
    sources = [[ids.index(j) for j in chosen[i]] for i in ids]
    assert all(len(s) >= 1 for s in sources)
    normals = C.depth_normals(depth, pose, rays, ray_index)["normals"]
    ref = C.fuse_depth_maps(depth, pose, cam, rays, ray_index, sources, normals, images[0].cpu().numpy()[ids], min_views=2)
    return ids, depth, ref


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("fusion")


def test_fused_cloud_is_the_restatement_on_the_read_back_maps(tmp):
    sc, rec, _, pred, before, _ = _run(tmp)
    ids, depth, ref = _restated(tmp)
    cloud = pred["fused_point_cloud"]
    assert isinstance(cloud, fusion.FusedCloud) and all(t.is_cuda for t in cloud)
    assert set(pred) == set(before) | {"fused_point_cloud"} and all(pred[k] is before[k] for k in before)    # no other key changes
    got = fusion.FusedCloud(*(t.cpu().numpy() for t in cloud))
    print(f"\n{len(got.xyz)} points (restatement {len(ref['xyz'])}) of {int((depth > 0).sum())} pixels with depth, per view "
          f"{ref['counts']}, seeds {ref['seeds']}, num_views {np.bincount(got.num_views).tolist()}; margins "
          f"{ {k: f'{v:.1e}' for k, v in ref['margins'].items()} }")
    assert len(got.xyz) == len(ref["xyz"]) > 0
    assert np.array_equal(got.view, np.asarray(ids, np.int32)[ref["view"]])                # `view` is the image id
    for k in ("pixel", "num_views", "xyz", "normal", "rgb"):
        assert getattr(got, k).tobytes() == ref[k].tobytes(), k


def test_points_name_pixels_with_depth_and_the_count_drops(tmp):
    sc, rec, _, pred, _, _ = _run(tmp)
    ids, depth, ref = _restated(tmp)
    got = fusion.FusedCloud(*(t.cpu().numpy() for t in pred["fused_point_cloud"]))
    H, W = depth.shape[1:]
    assert ((got.pixel >= 0) & (got.pixel < H * W)).all() and np.isin(got.view, ids).all()
    rows = np.searchsorted(ids, got.view)
    assert (depth.reshape(len(ids), -1)[rows, got.pixel] > 0).all()
    assert (got.num_views >= 2).all() and got.num_views.max() <= 5
    assert len(np.unique(rows.astype(np.int64) * H * W + got.pixel)) == len(got.pixel)
    with_depth = int((depth > 0).sum())
    print(f"\n{len(got.xyz)} fused points for {with_depth} pixels with depth: {len(got.xyz) / with_depth:.3f}")
    assert 0 < len(got.xyz) < with_depth
    assert np.isfinite(got.xyz).all() and np.isfinite(got.normal).all() and np.isfinite(got.rgb).all()


def test_distance_to_the_true_plane(tmp):
    """At 2 x what the restatement gives on the same read-back maps (CPU), never against the kernel's own output."""
    _, _, _, pred, _, _ = _run(tmp)
    _, _, ref = _restated(tmp)
    want = C.plane_distance(ref["xyz"])
    got = C.plane_distance(pred["fused_point_cloud"].xyz.cpu().numpy())
    angle = C.normal_angle_deg(pred["fused_point_cloud"].normal.cpu().numpy())
    print(f"\ndistance to the plane: median {np.median(got):.4e}, largest {got.max():.4e} (restatement: {np.median(want):.4e}, "
          f"{want.max():.4e}); normal against the plane's: median {np.nanmedian(angle):.3f} deg, largest {np.nanmax(angle):.3f} deg")
    assert got.max() <= 2 * want.max() and np.median(got) <= 2 * np.median(want)


def test_wrong_arguments_raise_and_colours_are_optional(tmp):
    _, rec, images, pred, _, _ = _run(tmp)
    runner = GeometryRunner(GeometryConfig())
    start = {"reconstruction": rec, "depth_dict": pred["depth_dict"]}
    with pytest.raises(ValueError, match="view_order"):
        runner.fuse_dense_point_cloud(dict(start), images, view_order=[0, 1])
    with pytest.raises(ValueError, match="images must be"):
        runner.fuse_dense_point_cloud(dict(start), images[..., :-1].contiguous())
    with pytest.raises(ValueError, match="has no frame"):
        runner.fuse_dense_point_cloud(dict(start), images[:, :-1].contiguous())
    plain = runner.fuse_dense_point_cloud(dict(start), None)["fused_point_cloud"]
    assert torch.equal(plain.xyz, pred["fused_point_cloud"].xyz) and not plain.rgb.any()
    assert torch.equal(plain.normal, pred["fused_point_cloud"].normal)


def test_ply_reads_back_to_the_cloud(tmp):
    _, _, _, pred, _, path = _run(tmp)
    cloud = pred["fused_point_cloud"]
    back = fusion.read_ply(path)
    assert back.xyz.tobytes() == cloud.xyz.cpu().numpy().tobytes()
    assert back.normal.tobytes() == cloud.normal.cpu().numpy().tobytes()
    assert np.array_equal(back.num_views, cloud.num_views.cpu().numpy())
    assert np.abs(back.rgb.astype(np.float64) - np.clip(cloud.rgb.cpu().numpy(), 0, 1)).max() <= 0.5 / 255 + 1e-7
