"""Frames and a sparse reconstruction in, dense depth out, with no learned part: GeometryRunner.dense_reconstruct_from_frames
on the analytic scene of tests/mvs_cases.py -- 6 frames of 48 x 64 under one SIMPLE_RADIAL camera (k = 0.08) on a line of
2.5 units in front of the slanted plane, the reconstruction built by batch_matrix_to_pycolmap from the true cameras and 400
points on the plane (181 of them seen by two views or more), 24 planes, every other option at its default.

Bounds.  The inverse-depth error of the surviving pixels against the analytic depth, in plane spacings of the image's own
range, per image: median and 90th percentile within 2 x mvs_cases.TRUTH_MEDIAN / TRUTH_P90, the bound of
tests/test_mvs_host.py.  The surviving share: the consistency check cannot keep a pixel that fewer than two sources see, so
the share of pixels that pass the check on the TRUE depth maps (the restated filter, on the CPU) is what exact depths would
reach; the run from frames must keep half of it over all images -- the factor 2 of the other bounds.  Every figure is
printed before it is asserted.

Measured (one MI355X): surviving 0.417 .. 0.694 per image, 0.579 overall, against 0.942 on the true maps (bound 0.471);
median 0.089 .. 0.371 and 90th percentile 0.244 .. 0.839 spacings (bounds 0.665 and 2.091).  The first frames see the
plane at 29 degrees and carry the fronto-parallel bias of the sweep (1.2 % of the depth in the median), which the 1 % check
then thins out; slanted hypotheses are not in this change."""
import functools

import numpy as np
import pytest
import torch

from tests import mvs_cases as C
from vggsfm_amd import mvs
from vggsfm_amd.runners import GeometryConfig, GeometryRunner
from vggsfm_amd.utils.tensor_to_pycolmap import batch_matrix_to_pycolmap

pytestmark = pytest.mark.gpu

PLANES = 24


@functools.lru_cache(maxsize=None)
def _run():
    sc = C.reconstruction_scene()
    S, H, W = sc["frames"].shape
    K = np.zeros((S, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = sc["cams"][:, 0]
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = sc["cams"][:, 1], sc["cams"][:, 2], 1.0
    rec = batch_matrix_to_pycolmap(sc["points3D"], sc["poses"], K, sc["tracks"], sc["masks"], np.array([W, H]),
                                   shared_camera=True, camera_type="SIMPLE_RADIAL", extra_params=sc["cams"][:, 3:4])
    assert rec.num_reg_images() == S and rec.num_points3D() > 150
    images = torch.from_numpy(sc["frames"]).cuda()[None, :, None].expand(1, S, 3, H, W).contiguous()
    pred = GeometryRunner(GeometryConfig(visual_dense_point_cloud=True)).dense_reconstruct_from_frames(
        {"reconstruction": rec}, images, num_planes=PLANES)
    return sc, rec, images, pred


def _spacings(rec):
    return {n: (1.0 / near - 1.0 / far) / (PLANES - 1) for n, (near, far) in mvs.depth_ranges(rec).items()}


def test_keys_shapes_and_zeros():
    sc, rec, images, pred = _run()
    S, H, W = sc["frames"].shape
    names = [f"image_{s}" for s in range(S)]
    assert sorted(pred["depth_dict"]) == sorted(pred["depth_conf_dict"]) == names
    ranges = mvs.depth_ranges(rec)
    for n in names:
        d, c = pred["depth_dict"][n], pred["depth_conf_dict"][n]
        assert d.is_cuda and c.is_cuda and d.dtype == c.dtype == torch.float32 and d.shape == c.shape == (H, W)
        d, c = d.cpu().numpy(), c.cpu().numpy()
        near, far = ranges[n]
        assert np.isfinite(d).all() and np.isfinite(c).all() and ((d == 0) | ((d >= near * 0.99) & (d <= far * 1.01))).all()
        assert (d[c < 0.5] == 0).all()                                       # under min_conf: no depth
    # without the point cloud: the key is there and None, as align_dense_depth_maps leaves it
    plain = GeometryRunner(GeometryConfig()).dense_reconstruct_from_frames({"reconstruction": rec}, images, num_planes=PLANES)
    assert plain["unproj_dense_points3D"] is None
    for n in names:
        assert torch.equal(plain["depth_dict"][n], pred["depth_dict"][n])


def test_depth_against_truth_and_surviving_share():
    sc, rec, _, pred = _run()
    S = sc["frames"].shape[0]
    dw = _spacings(rec)
    sources = mvs.select_source_views(rec)
    truth32 = sc["truth"].astype(np.float32)
    kept, visible = [], []
    for s in range(S):
        n = f"image_{s}"
        d = pred["depth_dict"][n].cpu().numpy()
        v = d > 0
        err = np.abs(1.0 / d[v].astype(np.float64) - 1.0 / sc["truth"][s][v]) / dw[n]
        on_truth = C.consistency_filter(truth32, sc["poses"], sc["cams"], sc["rays"], sc["ray_index"], s, sources[s], 0.01, 1.0, 2)
        kept.append(v.mean())
        visible.append((on_truth["depth"] > 0).mean())
        print(f"{n}: sources {sources[s]}, surviving {kept[-1]:.4f} (true maps: {visible[-1]:.4f}), median {np.median(err):.4f}, "
              f"90th percentile {np.percentile(err, 90):.4f} spacings, relative median {np.median(np.abs(d[v] / sc['truth'][s][v] - 1)):.5f}")
        assert v.any() and np.median(err) <= 2 * C.TRUTH_MEDIAN and np.percentile(err, 90) <= 2 * C.TRUTH_P90
    print(f"surviving share over all images {np.mean(kept):.4f}, on the true maps {np.mean(visible):.4f}")
    assert np.mean(kept) >= 0.5 * np.mean(visible)


def test_point_cloud_format_and_distance_to_the_plane():
    """unproj_dense_points3D[name] = np.array([xyz, rgb]) as align_dense_depth_maps writes it: the points of the pixels with
    depth, row-major; each projects back to its pixel, and its depth error is that of the map."""
    sc, rec, images, pred = _run()
    dw = _spacings(rec)
    cloud = pred["unproj_dense_points3D"]
    assert sorted(cloud) == sorted(pred["depth_dict"])
    for s in range(sc["frames"].shape[0]):
        n = f"image_{s}"
        d = pred["depth_dict"][n].cpu().numpy()
        ys, xs = np.nonzero(d)
        arr = cloud[n]
        assert isinstance(arr, np.ndarray) and arr.dtype == np.float64 and arr.shape == (2, len(ys), 3)
        xyz, rgb = arr
        uv, z = C.project(sc["poses"][s], sc["cams"][s], xyz)
        assert np.abs(uv - np.stack([xs, ys], -1)).max() < 1e-6
        assert np.allclose(rgb, images[0, s].permute(1, 2, 0).cpu().numpy()[ys, xs])
        err = np.abs(1.0 / z - 1.0 / sc["truth"][s][ys, xs]) / dw[n]
        p0, _, _, nrm = C._plane()
        print(f"{n}: {len(ys)} points, median {np.median(err):.4f} spacings, median distance to the plane "
              f"{np.median(np.abs((xyz - p0) @ nrm)):.4f}")
        assert np.median(err) <= 2 * C.TRUTH_MEDIAN and np.percentile(err, 90) <= 2 * C.TRUTH_P90


def test_wrong_frame_size_and_camera_model_raise():
    import copy
    _, rec, images, _ = _run()
    runner = GeometryRunner(GeometryConfig())
    with pytest.raises(ValueError, match="frames are 48 x 63"):
        runner.dense_reconstruct_from_frames({"reconstruction": rec}, images[..., :-1].contiguous())
    with pytest.raises(ValueError, match="has no frame"):
        runner.dense_reconstruct_from_frames({"reconstruction": rec}, images[:, :-1].contiguous())
    other = copy.deepcopy(rec)
    for cam in other.cameras.values():
        cam.model = "PINHOLE"
    with pytest.raises(NotImplementedError, match="PINHOLE"):
        runner.dense_reconstruct_from_frames({"reconstruction": other}, images)
