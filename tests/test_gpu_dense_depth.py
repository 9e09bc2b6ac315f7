"""Dense depth alignment on the MI355X against the reference's dense_depth stage (runner.py:744-814, utils.py:635-770,
scikit-learn 1.7), recorded in tests/golden/dense_depth_*.npz by scripts/make_golden_dense_depth.py."""
import math
import os

import numpy as np
import pytest
import torch

from vggsfm_amd import dense_depth as DD
from vggsfm_amd import pycolmap_compat as pc
from vggsfm_amd.runners import GeometryConfig, GeometryRunner
from vggsfm_amd.utils.utils import align_dense_depth_maps

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["pinhole", "radial_shared", "low_inlier"]


def _golden(case):
    return np.load(os.path.join(GOLD, f"dense_depth_{case}.npz"), allow_pickle=False)


def _reconstruction(g):
    """The compat reconstruction the golden script built (cameras scaled to the small maps, optional empty image)."""
    S, camera, shared = int(g["S"]), str(g["camera"]), bool(g["shared"])
    extra = g["extra_params"] if camera == "SIMPLE_RADIAL" else None
    rec = pc.Reconstruction.from_arrays(g["points3D"], g["extrinsics"], g["intrinsics"], g["tracks"], g["mask"],
                                        np.array([1024, 1024]), shared_camera=shared, camera_type=camera,
                                        extra_params=extra)
    for c in rec.cameras.values():
        c._params[:3] /= float(g["scale"])
        c.width = c.height = int(round(1024 / float(g["scale"])))
    if bool(g["empty_image"]):
        cam = next(iter(rec.cameras.values()))
        rec.add_image(pc.Image(S, f"image_{S}", cam.camera_id, rec.images[0].cam_from_world))
    return rec


def _names(g):
    return [str(n) for n in g["names"]]


def _packed_inputs(g):
    names = _names(g)
    maps = [g[f"disp_in_{k}"].copy() for k in range(len(names))]
    uvds = [g[f"uvd_{k}"] for k in range(len(names))]
    obs_ptr = np.concatenate([[0], np.cumsum([len(u) for u in uvds])]).astype(np.int64)
    uvd = torch.from_numpy(np.concatenate(uvds)).cuda()
    return names, maps, uvd, obs_ptr


def _yscale(g, k):
    """Typical inverse depth of image k: the scale of the fitted disparities."""
    return float(np.median(1.0 / np.clip(g[f"uvd_{k}"][:, 2], 1e-4, 1e4)))


def _check_maps(depth, disp, g, k):
    """End-to-end maps against the reference's.  The fit agrees with scikit-learn's float32 refit to ~1e-6 of the fitted
    disparities (its intercept cancels, mean(y) - coef * mean(x)), so the rescaled disparities are compared on that scale;
    the depth is their float32 inverse bit for bit, and within 1e-5 of the reference's wherever the disparity is not tiny.
    The zero pattern is the reference's except for pixels within 1e-5 of the (0, 1e4] bounds."""
    ref_depth, ref_disp = g[f"depth_{k}"], g[f"disp_out_{k}"]
    depth = depth.cpu().numpy() if torch.is_tensor(depth) else depth
    disp = disp.cpu().numpy() if torch.is_tensor(disp) else disp
    assert depth.dtype == np.float32 and depth.shape == ref_depth.shape
    resc = g[f"disp_in_{k}"] * g[f"coef_{k}"][0] + g[f"intercept_{k}"]          # before the (0, 1e4] check
    near = (np.abs(resc) < 1e-5) | (np.abs(resc - 1e4) < 1e-5 * 1e4)
    assert np.array_equal((depth == 0)[~near], (ref_depth == 0)[~near])
    ys = _yscale(g, k)
    np.testing.assert_allclose(disp, ref_disp, rtol=1e-6, atol=2e-6 * ys)
    inv = np.zeros_like(disp)
    np.divide(np.float32(1), disp, out=inv, where=disp != 0)
    inv[np.isinf(inv)] = 0
    assert np.array_equal(depth.view(np.int32), inv.view(np.int32))
    big = (depth != 0) & (ref_depth != 0) & (np.abs(ref_disp) > 0.1 * ys)
    np.testing.assert_allclose(depth[big], ref_depth[big], rtol=1e-5)


@pytest.mark.parametrize("case", CASES)
def test_sparse_depth_matches_reference(case):
    g = _golden(case)
    pred = GeometryRunner(GeometryConfig()).extract_sparse_depth_and_point_from_reconstruction(
        {"reconstruction": _reconstruction(g)})
    names = _names(g)
    assert list(pred["sparse_depth"]) == names == list(pred["sparse_point"])      # image with no observation: no key
    for k, n in enumerate(names):
        uvd, xyzid = pred["sparse_depth"][n], pred["sparse_point"][n]
        assert uvd.shape == g[f"uvd_{k}"].shape and xyzid.shape == g[f"xyzid_{k}"].shape
        assert np.array_equal(xyzid[:, 3], g[f"xyzid_{k}"][:, 3])                  # same ids, same order
        assert np.array_equal(xyzid[:, :3], g[f"xyzid_{k}"][:, :3])
        np.testing.assert_allclose(uvd, g[f"uvd_{k}"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", CASES)
def test_align_replays_sklearn_draws(case):
    g = _golden(case)
    names, maps, uvd, obs_ptr = _packed_inputs(g)
    packed = DD.pack_maps(maps)
    res = DD.align(packed, uvd, obs_ptr, samples=[g[f"draws_{k}"] for k in range(len(names))])
    status, n_trials = res.status.cpu().numpy(), res.n_trials.cpu().numpy()
    kept, inlier = res.kept.cpu().numpy().astype(bool), res.inlier.cpu().numpy().astype(bool)
    scale, shift = res.scale.cpu().numpy(), res.shift.cpu().numpy()
    for k in range(len(names)):
        a, b = obs_ptr[k], obs_ptr[k + 1]
        assert status[k] == 0
        assert n_trials[k] == int(g[f"n_trials_{k}"]), (k, n_trials[k], int(g[f"n_trials_{k}"]))
        mask = g[f"inlier_mask_{k}"]
        assert kept[a:b].sum() == len(mask)
        assert np.array_equal(inlier[a:b][kept[a:b]], mask)
        assert not inlier[a:b][~kept[a:b]].any()
        coef, icpt = float(g[f"coef_{k}"][0]), float(g[f"intercept_{k}"])
        if coef == 0.0:
            assert scale[k] == 0.0
        else:
            assert abs(scale[k] - coef) <= 1e-6 * abs(coef), (k, scale[k], coef)
        # intercept = mean(y) - coef * mean(x) cancels: scikit-learn's float32 refit carries ~1e-7 of mean(y) in it, so it
        # is compared on the scale of the fitted values
        y_mean = float(np.mean(1.0 / np.clip(g[f"uvd_{k}"][kept[a:b], 2], 1e-4, 1e4)))
        assert abs(shift[k] - icpt) <= 2e-6 * max(abs(icpt), y_mean), (k, shift[k], icpt, y_mean)


@pytest.mark.parametrize("case", CASES)
def test_apply_and_unproject_bit_exact_with_reference_fit(case):
    g = _golden(case)
    names, maps, _, _ = _packed_inputs(g)
    packed = DD.pack_maps(maps)
    scale = torch.tensor([float(g[f"coef_{k}"][0]) for k in range(len(names))], dtype=torch.float32).cuda()
    shift = torch.tensor([float(g[f"intercept_{k}"]) for k in range(len(names))], dtype=torch.float32).cuda()
    depth = DD.apply(packed, scale, shift)
    off = packed.off.cpu().numpy()
    flat, dflat = packed.flat.cpu().numpy(), depth.cpu().numpy()
    for k in range(len(names)):
        h, w = maps[k].shape
        d, z = flat[off[k]:off[k + 1]].reshape(h, w), dflat[off[k]:off[k + 1]].reshape(h, w)
        assert d.dtype == np.float32 and z.dtype == np.float32
        assert np.array_equal(d.view(np.int32), g[f"disp_out_{k}"].view(np.int32)), k
        assert np.array_equal(z.view(np.int32), g[f"depth_{k}"].view(np.int32)), k
    rec = _reconstruction(g)
    ids = {rec.images[i].name: i for i in rec.images}
    pose, cam = DD._camera_rows(rec, [ids[n] for n in names])
    inv = [rec.images[ids[n]].cam_from_world.inverse() for n in names]
    inv_pose = np.stack([np.concatenate([t.rotation.matrix(), t.translation[:, None]], axis=1) for t in inv])
    xyz, counts = DD.unproject(packed, depth, cam, inv_pose)
    xyz, start = xyz.cpu().numpy(), np.concatenate([[0], np.cumsum(counts.cpu().numpy())])
    for k in range(len(names)):
        ref = g[f"cloud_xyz_{k}"]
        got = xyz[start[k]:start[k + 1]]
        assert got.shape == ref.shape
        np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())


@pytest.mark.parametrize("case", CASES)
def test_align_dense_depth_maps_end_to_end(case):
    g = _golden(case)
    names = _names(g)
    rec = _reconstruction(g)
    sparse_depth = {n: list(g[f"uvd_{k}"]) for k, n in enumerate(names)}       # the reference's lists of 1-D arrays
    disp = {n: g[f"disp_in_{k}"].copy() for k, n in enumerate(names)}
    rgb = {n: g[f"rgb_{k}"] for k, n in enumerate(names)}
    depth_dict, cloud = align_dense_depth_maps(rec, sparse_depth, disp, rgb, visual_dense_point_cloud=True,
                                               samples={n: g[f"draws_{k}"] for k, n in enumerate(names)})
    assert list(depth_dict) == names == list(cloud)
    for k, n in enumerate(names):
        ref, got = g[f"depth_{k}"], depth_dict[n]
        _check_maps(got, disp[n], g, k)                                             # disp: mutated in place
        if np.array_equal(got == 0, ref == 0):
            assert cloud[n].shape == (2,) + g[f"cloud_xyz_{k}"].shape
            # the reference's colour half: rgb / 255 over its valid pixels (checked against it by the golden script)
            valid = (g[f"disp_out_{k}"] != 0).reshape(-1)
            assert np.array_equal(cloud[n][1], (g[f"rgb_{k}"] / 255.0).reshape(-1, 3)[valid])
            sel = (np.abs(g[f"disp_out_{k}"]) > 0.1 * _yscale(g, k)).reshape(-1)[(ref != 0).reshape(-1)]
            np.testing.assert_allclose(cloud[n][0][sel], g[f"cloud_xyz_{k}"][sel], rtol=1e-5,
                                       atol=1e-5 * np.abs(g[f"cloud_xyz_{k}"]).max())


def test_device_tensors_in_and_out():
    g = _golden("pinhole")
    names = _names(g)
    rec = _reconstruction(g)
    sparse_depth = {n: g[f"uvd_{k}"] for k, n in enumerate(names)}
    disp = {n: torch.from_numpy(g[f"disp_in_{k}"].copy()).cuda() for k, n in enumerate(names)}
    depth_dict, cloud = align_dense_depth_maps(rec, sparse_depth, disp, {}, samples=[g[f"draws_{k}"] for k in range(len(names))])
    assert cloud is None
    for k, n in enumerate(names):
        assert depth_dict[n].is_cuda and depth_dict[n].dtype == torch.float32
        _check_maps(depth_dict[n], disp[n], g, k)


def test_on_device_draws_recover_a_known_line():
    rng = np.random.default_rng(3)
    H, W, n = 64, 80, 1500
    a_true, b_true = 0.8, 0.3
    u, v = rng.integers(0, W, n), rng.integers(0, H, n)
    u, v = u.astype(np.float64) + rng.uniform(-0.4, 0.4, n), v.astype(np.float64) + rng.uniform(-0.4, 0.4, n)
    disp_px = rng.uniform(5.0, 40.0, n)
    inl = rng.uniform(size=n) < 0.4
    y = np.where(inl, a_true * disp_px + b_true + rng.normal(0, 1e-3, n), rng.uniform(5.0, 200.0, n))
    # one observation per pixel so that the sampled disparity is the one the line was built on
    _, first = np.unique(np.round(v).astype(int) * W + np.round(u).astype(int), return_index=True)
    keep = np.zeros(n, bool)
    keep[first] = True
    dm = np.zeros((H, W), np.float32)
    dm[np.round(v[keep]).astype(int), np.round(u[keep]).astype(int)] = disp_px[keep].astype(np.float32)
    uvd = np.stack([u[keep], v[keep], 1.0 / y[keep]], 1)
    packed = DD.pack_maps([dm])
    res = DD.align(packed, torch.from_numpy(uvd).cuda(), np.array([0, len(uvd)], np.int64), seed=1234)
    assert int(res.status[0]) == 0
    scale, shift = float(res.scale[0]), float(res.shift[0])
    assert abs(scale - a_true) < 1e-3 and abs(shift - b_true) < 3e-2, (scale, shift)
    M, n_in, n_trials = int(res.n_kept[0]), int(res.n_inliers[0]), int(res.n_trials[0])
    bound = abs(math.ceil(math.log(max(2.220446049250313e-16, 1 - 0.99)) /
                          math.log(max(2.220446049250313e-16, 1 - (n_in / M) ** 2))))
    assert n_trials == bound, (n_trials, bound, n_in, M)
    res2 = DD.align(packed, torch.from_numpy(uvd).cuda(), np.array([0, len(uvd)], np.int64), seed=1234)
    assert float(res2.scale[0]) == scale and int(res2.n_trials[0]) == n_trials          # reproducible per seed


def test_errors_match_reference():
    g = _golden("pinhole")
    names = _names(g)
    rec = _reconstruction(g)
    disp = {n: g[f"disp_in_{k}"].copy() for k, n in enumerate(names)}
    sparse_depth = {n: g[f"uvd_{k}"] for k, n in enumerate(names)}
    sparse_depth[names[2]] = []
    with pytest.raises(ValueError, match="Too few points for depth alignment"):
        align_dense_depth_maps(rec, sparse_depth, disp, {}, samples={n: g[f"draws_{k}"] for k, n in enumerate(names)})
    # the reference's loop rescaled the maps before the failing image, and only those
    for k, n in enumerate(names):
        if k < 2:
            np.testing.assert_allclose(disp[n], g[f"disp_out_{k}"], rtol=1e-6, atol=2e-6 * _yscale(g, k))
        else:
            assert np.array_equal(disp[n], g[f"disp_in_{k}"])
    bad = {n: g[f"uvd_{k}"].copy() for k, n in enumerate(names)}
    bad[names[0]][:, 2] = np.nan
    with pytest.raises(ValueError):
        align_dense_depth_maps(rec, bad, {n: g[f"disp_in_{k}"].copy() for k, n in enumerate(names)}, {})


def test_runner_dense_reconstruct():
    g = _golden("radial_shared")
    names = _names(g)
    runner = GeometryRunner(GeometryConfig(visual_dense_point_cloud=True))
    pred = runner.extract_sparse_depth_and_point_from_reconstruction({"reconstruction": _reconstruction(g)})
    disp = {n: g[f"disp_in_{k}"].copy() for k, n in enumerate(names)}
    rgb = {n: g[f"rgb_{k}"] for k, n in enumerate(names)}
    pred = runner.dense_reconstruct(pred, [f"/x/{n}" for n in names], rgb, disp,
                                    samples={n: g[f"draws_{k}"] for k, n in enumerate(names)})
    assert list(pred["depth_dict"]) == names == list(pred["unproj_dense_points3D"])
    for k, n in enumerate(names):
        _check_maps(pred["depth_dict"][n], disp[n], g, k)
        assert pred["unproj_dense_points3D"][n].shape[0] == 2
