"""The 6-frame 48 x 64 run of tests/test_gpu_mvs_reconstruct.py through GeometryRunner.dense_reconstruct_from_frames with
patchmatch_iterations = 4 (sweep, PatchMatch refinement, consistency check on the REFINED maps), beside the same run with
patchmatch_iterations = 0 -- the parent's path, computed in this test -- and without the option.

Bounds.  Per image, median and 90th percentile of the inverse-depth error of the surviving pixels in plane spacings of the
image's own range: section 28's, 2 x mvs_cases.TRUTH_MEDIAN / TRUTH_P90 = 0.665 / 2.091.  Against the parent's path: the
surviving share over all images is not below it; the two frames that see the plane at about 29 degrees (image_0, image_1)
have a lower median than they have there; the fused cloud, with the refined normals, is in the median not further from the
true plane.  With patchmatch_iterations = 0, predictions is what it is without the option, bit for bit.  Every figure is
printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from tests import fusion_cases as F
from tests import mvs_cases as C
from vggsfm_amd import mvs
from vggsfm_amd.runners import GeometryConfig, GeometryRunner
from vggsfm_amd.utils.tensor_to_pycolmap import batch_matrix_to_pycolmap

pytestmark = pytest.mark.gpu

PLANES, ITERATIONS = 24, 4


@functools.lru_cache(maxsize=None)
def _run():
    sc = C.reconstruction_scene()
    S, H, W = sc["frames"].shape
    K = np.zeros((S, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = sc["cams"][:, 0]
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = sc["cams"][:, 1], sc["cams"][:, 2], 1.0
    rec = batch_matrix_to_pycolmap(sc["points3D"], sc["poses"], K, sc["tracks"], sc["masks"], np.array([W, H]),
                                   shared_camera=True, camera_type="SIMPLE_RADIAL", extra_params=sc["cams"][:, 3:4])
    assert rec.num_reg_images() == S
    images = torch.from_numpy(sc["frames"]).cuda()[None, :, None].expand(1, S, 3, H, W).contiguous()
    runner = GeometryRunner(GeometryConfig(visual_dense_point_cloud=True))
    plain = runner.dense_reconstruct_from_frames({"reconstruction": rec}, images, num_planes=PLANES)
    parent = runner.dense_reconstruct_from_frames({"reconstruction": rec}, images, num_planes=PLANES, patchmatch_iterations=0)
    refined = runner.dense_reconstruct_from_frames({"reconstruction": rec}, images, num_planes=PLANES,
                                                   patchmatch_iterations=ITERATIONS)
    return sc, rec, images, runner, plain, parent, refined


def _errors(sc, rec, pred):
    """per image: surviving share, median and 90th percentile of the inverse-depth error in the image's plane spacings"""
    dw = {n: (1.0 / near - 1.0 / far) / (PLANES - 1) for n, (near, far) in mvs.depth_ranges(rec).items()}
    rows = []
    for s in range(sc["frames"].shape[0]):
        n = f"image_{s}"
        d = pred["depth_dict"][n].cpu().numpy()
        v = d > 0
        err = np.abs(1.0 / d[v].astype(np.float64) - 1.0 / sc["truth"][s][v]) / dw[n]
        rows.append((float(v.mean()), float(np.median(err)), float(np.percentile(err, 90))))
    return rows


def test_zero_iterations_is_the_parents_path_bit_for_bit():
    _, _, _, _, plain, parent, _ = _run()
    assert list(plain) == list(parent) and "depth_normal_dict" not in parent
    for key in ("depth_dict", "depth_conf_dict"):
        assert list(plain[key]) == list(parent[key])
        for n in plain[key]:
            assert torch.equal(plain[key][n], parent[key][n]), (key, n)
    assert list(plain["unproj_dense_points3D"]) == list(parent["unproj_dense_points3D"])
    for n, arr in plain["unproj_dense_points3D"].items():
        assert arr.tobytes() == parent["unproj_dense_points3D"][n].tobytes(), n
    assert plain["reconstruction"] is parent["reconstruction"]


def test_keys_shapes_and_zeros():
    sc, rec, _, _, plain, _, refined = _run()
    S, H, W = sc["frames"].shape
    names = [f"image_{s}" for s in range(S)]
    assert set(refined) == set(plain) | {"depth_normal_dict"}
    assert sorted(refined["depth_dict"]) == sorted(refined["depth_conf_dict"]) == sorted(refined["depth_normal_dict"]) == names
    for n in names:
        d, c, nm = refined["depth_dict"][n], refined["depth_conf_dict"][n], refined["depth_normal_dict"][n]
        assert d.is_cuda and d.dtype == c.dtype == nm.dtype == torch.float32 and d.shape == c.shape == (H, W) and nm.shape == (H, W, 3)
        d, c, nm = d.cpu().numpy(), c.cpu().numpy(), nm.cpu().numpy()
        assert np.isfinite(d).all() and np.isfinite(c).all() and np.isfinite(nm).all() and (d[c < 0.5] == 0).all()
        assert (nm[d == 0] == 0).all() and np.abs(np.linalg.norm(nm[d > 0].astype(np.float64), axis=-1) - 1.0).max() < 1e-6
        assert refined["unproj_dense_points3D"][n].shape == (2, int((d > 0).sum()), 3)


def test_depth_against_truth_and_against_the_parents_path():
    sc, rec, _, _, _, parent, refined = _run()
    before, after = _errors(sc, rec, parent), _errors(sc, rec, refined)
    for s, (b, a) in enumerate(zip(before, after)):
        print(f"image_{s}: surviving {b[0]:.4f} -> {a[0]:.4f}, median {b[1]:.4f} -> {a[1]:.4f}, 90th percentile {b[2]:.4f} -> {a[2]:.4f} spacings")
    kept_before, kept_after = np.mean([b[0] for b in before]), np.mean([a[0] for a in after])
    print(f"surviving share over all images {kept_before:.4f} -> {kept_after:.4f}")
    for a in after:
        assert a[0] > 0 and a[1] <= 2 * C.TRUTH_MEDIAN and a[2] <= 2 * C.TRUTH_P90
    assert kept_after >= kept_before
    for s in (0, 1):                                                       # the frames section 28 names as biased
        assert after[s][1] < before[s][1]


def test_fused_cloud_with_the_refined_normals():
    sc, rec, images, runner, _, parent, refined = _run()
    ids = sorted(int(i) for i in rec.reg_image_ids())
    normals = torch.stack([refined["depth_normal_dict"][rec.images[i].name] for i in ids])
    keys = set(refined)
    mine = runner.fuse_dense_point_cloud(dict(refined), images, normals=normals)["fused_point_cloud"]
    theirs = runner.fuse_dense_point_cloud(dict(parent), images)["fused_point_cloud"]
    assert set(refined) == keys
    d_mine, d_theirs = F.plane_distance(mine.xyz.cpu().numpy()), F.plane_distance(theirs.xyz.cpu().numpy())
    a_mine, a_theirs = F.normal_angle_deg(mine.normal.cpu().numpy()), F.normal_angle_deg(theirs.normal.cpu().numpy())
    print(f"\nfused cloud: {len(theirs.xyz)} -> {len(mine.xyz)} points, median distance to the plane {np.median(d_theirs):.4e} -> "
          f"{np.median(d_mine):.4e}, median normal angle {np.nanmedian(a_theirs):.3f} -> {np.nanmedian(a_mine):.3f} degrees")
    assert len(mine.xyz) > 0 and np.isfinite(mine.xyz.cpu().numpy()).all() and np.isfinite(mine.normal.cpu().numpy()).all()
    assert np.median(d_mine) <= np.median(d_theirs)
