"""Sim(3) alignment and pose metrics, the part that needs no GPU: argument validation before any launch, the Sim3d algebra,
Reconstruction.transform and the shared-observation vote of align_reconstructions_via_points."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import sim3_cases as SC
from vggsfm_amd import _lib, sim3, video
from vggsfm_amd import pycolmap_compat as pc
from vggsfm_amd.scene import make_scene
from vggsfm_amd.utils import metric



def test_entries_refuse_bad_sizes_before_any_launch():
    L = _lib.lib()
    one = torch.zeros(4096, dtype=torch.float64)         # (host memory: nothing is launched on these paths)
    bad, workspace, unsupported = -1, -3, -4
    big = one.numel() * 8
    assert L.vggs_sim3_workspace_bytes(1, 250000, 1024) > L.vggs_sim3_workspace_bytes(1, 250000, 0) > 0
    assert L.vggs_sim3_workspace_bytes(0, 10, 10) == 0 and L.vggs_sim3_workspace_bytes(-1, 10, 10) == 0
    assert L.vggs_sim3_fit(one, one, None, -1, 8, 1, one, one, one, big, None) == bad
    assert L.vggs_sim3_fit(one, one, None, 1, -8, 1, one, one, one, big, None) == bad
    assert L.vggs_sim3_fit(None, one, None, 1, 8, 1, one, one, one, big, None) == bad
    assert L.vggs_sim3_fit(one, one, None, 1, 8, 1, one, None, one, big, None) == bad
    assert L.vggs_sim3_fit(None, None, None, 0, 8, 1, None, None, None, 0, None) == 0       # no problems: a no-op
    assert L.vggs_sim3_fit(None, None, None, 3, 0, 1, None, None, None, 0, None) == 0       # no points: a no-op
    assert L.vggs_sim3_fit(one, one, None, 1, 5000, 1, one, one, one, 16, None) == workspace
    assert L.vggs_sim3_fit(one, one, None, 70000, 8, 1, one, one, one, big, None) == unsupported
    score = lambda *a: L.vggs_sim3_score(*a)
    assert score(one, one, None, one, one, one, 1, 8, -2, one, one, one, big, None) == bad
    assert score(one, one, None, one, one, None, 1, 8, 2, one, one, one, big, None) == bad   # no thresholds
    assert score(one, one, None, one, None, one, 1, 8, 2, one, one, one, big, None) == bad   # no validity flags
    assert score(None, None, None, None, None, None, 1, 8, 0, None, None, None, 0, None) == 0
    assert score(one, one, None, one, one, one, 1, 8, 2, one, one, one, 16, None) == workspace
    assert score(one, one, None, one, one, one, 1, 8, 2, one, one, None, 0, None) == workspace
    ransac = lambda B, N, H, lo, mn, outs, ws, nbytes: L.vggs_sim3_ransac(one, one, None, one, one, B, N, H, lo, mn, 1, *outs, None, None,
                                                                         ws, nbytes, None)
    outs = (one,) * 7
    assert ransac(1, 8, 4, -1, 3, outs, one, big) == bad
    assert ransac(1, 8, 4, 2, 2, outs, one, big) == bad                                     # min_inliers below 3
    assert ransac(-1, 8, 4, 2, 3, outs, one, big) == bad
    assert ransac(1, 8, 4, 2, 3, (one,) * 6 + (None,), one, big) == bad
    assert ransac(1, 8, 0, 2, 3, (None,) * 7, None, 0) == 0
    assert ransac(1, 8, 4, 2, 3, outs, one, 16) == workspace
    assert L.vggs_sim3_ransac(one, one, None, one, one, 1, 8, 4, 2, 3, 1, *outs, one, None, one, big, None) == bad   # half a score table
    assert L.vggs_pose_pair_errors(one, one, -1, one, one, None) == bad
    assert L.vggs_pose_pair_errors(None, one, 4, one, one, None) == bad
    assert L.vggs_pose_pair_errors(None, None, 1, None, None, None) == 0                    # no pairs: a no-op
    assert L.vggs_pose_pair_errors(one, one, 70000, one, one, None) == unsupported
    with pytest.raises(ctypes.ArgumentError):
        L.vggs_sim3_fit(one, one, None, 1, 2 ** 31, 1, one, one, one, big, None)


def test_arguments_are_validated_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "lib", no_library)
    x = torch.zeros(2, 8, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"\(N,3\) or \(B,N,3\)"):
        sim3.estimate_sim3(x, x[:, :7])
    with pytest.raises(ValueError, match="weights"):
        sim3.estimate_sim3(x, x, weights=torch.ones(2, 7))
    with pytest.raises(RuntimeError, match="no CPU path"):
        sim3.estimate_sim3(x, x)
    with pytest.raises(ValueError, match="min_inliers"):
        sim3.estimate_sim3_robust(x, x, 0.1, min_inliers=2)
    with pytest.raises(ValueError, match="lo_rounds"):
        sim3.estimate_sim3_robust(x, x, 0.1, lo_rounds=-1)
    with pytest.raises(ValueError, match="at least 3"):
        sim3.estimate_sim3_robust(x[:, :2], x[:, :2], 0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sim3.estimate_sim3_robust(x, x, 0.1)
    with pytest.raises(ValueError, match=r"\(S,3,4\)"):
        metric.pose_pair_errors(torch.zeros(4, 3, 4), torch.zeros(5, 3, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        metric.pose_pair_errors(torch.zeros(4, 3, 4), torch.zeros(4, 3, 4))


# --- Sim3d ----------------------------------------------------------------------------------------------------------------
def _random_sim3d(rng):
    return pc.Sim3d(float(rng.uniform(0.3, 3.0)), pc.Rotation3d(SC.random_rotation(rng)), rng.normal(size=3))


def test_sim3d_algebra():
    rng = np.random.default_rng(3)
    a, b = _random_sim3d(rng), _random_sim3d(rng)
    p = rng.normal(size=(5, 3))
    assert a.matrix().shape == (3, 4) and np.allclose(a.matrix()[:, :3], a.scale * a.rotation.matrix())
    assert np.allclose(a * p, a.scale * p @ a.rotation.matrix().T + a.translation, atol=1e-14)
    assert np.allclose(a * p[0], (a * p)[0], atol=1e-14)
    assert np.allclose(a.inverse() * (a * p), p, atol=1e-13) and np.allclose((a * a.inverse()).matrix(), np.eye(3, 4), atol=1e-14)
    assert np.allclose((a * b) * p, a * (b * p), atol=1e-13)
    assert np.allclose(pc.Sim3d().matrix(), np.eye(3, 4))
    # transform_camera_world = transform_extrinsics = the reference's apply_transformation with (R^T, -R^T t, s)
    ext = np.stack([np.concatenate([SC.random_rotation(rng), rng.normal(size=(3, 1))], axis=1) for _ in range(4)])
    by_class = np.stack([a.transform_camera_world(pc.Rigid3d(ext[i])).matrix() for i in range(4)])
    s, R, t = torch.tensor(a.scale, dtype=torch.float64), torch.from_numpy(a.rotation.matrix()), torch.from_numpy(a.translation)
    by_tensor = sim3.transform_extrinsics(torch.from_numpy(ext), s, R, t).numpy()
    by_align = video.apply_transformation(torch.from_numpy(ext), R.t()[None], (-R.t() @ t)[None], a.scale).numpy()
    assert np.allclose(by_class, by_tensor, atol=1e-14) and np.allclose(by_class, by_align, atol=1e-14)
    # a camera keeps seeing what it saw, up to the scale of its own frame
    x_cam = p @ ext[0, :, :3].T + ext[0, :, 3]
    moved = sim3.transform_points(torch.from_numpy(p), s, R, t).numpy()
    assert np.allclose(moved, a * p, atol=1e-14)
    assert np.allclose(moved @ by_class[0, :, :3].T + by_class[0, :, 3], a.scale * x_cam, atol=1e-13)
    assert np.allclose(sim3.camera_centers(torch.from_numpy(by_class)).numpy(),
                       a * sim3.camera_centers(torch.from_numpy(ext)).numpy(), atol=1e-13)


def _scene_reconstruction(seed=5):
    scn = make_scene(6, 120, "SIMPLE_RADIAL", shared_camera=True, seed=seed, outlier_frac=0.0)
    size = np.array([scn.image_size, scn.image_size])
    return pc.Reconstruction.from_arrays(scn.points3D, scn.extrinsics, scn.intrinsics, scn.tracks, scn.mask, size, 3000, True,
                                         "SIMPLE_RADIAL", scn.extra_params)


def _reprojections(rec):
    out = []
    for i in sorted(rec.images):
        im = rec.images[i]
        cam = rec.cameras[im.camera_id]
        pid = im.points2D._pid
        k = np.nonzero(pid >= 0)[0]
        out.append(np.stack([cam.img_from_cam(im.cam_from_world * rec._xyz[pid[j] - 1]) for j in k]))
    return np.concatenate(out)


def test_reconstruction_transform_keeps_every_reprojection(tmp_path):
    rec = _scene_reconstruction()
    before = _reprojections(rec)
    assert len(before) > 300
    T = _random_sim3d(np.random.default_rng(8))
    moved = copy.deepcopy(rec)
    moved.transform(T)
    assert np.abs(_reprojections(moved) - before).max() < 1e-9
    assert np.allclose(moved._xyz[:moved._n], T * rec._xyz[:rec._n], atol=1e-12)
    i = rec.reg_image_ids()[2]
    assert np.allclose(moved.images[i].projection_center(), T * rec.images[i].projection_center(), atol=1e-12)
    moved.write(str(tmp_path))
    back = pc.Reconstruction(str(tmp_path))
    assert np.array_equal(back._xyz[:back._n], moved._xyz[:moved._n])
    # (the file holds quaternions: the rotations come back to rounding)
    assert all(np.allclose(back.images[k].cam_from_world.matrix(), moved.images[k].cam_from_world.matrix(), atol=1e-13) for k in moved.images)
    assert np.abs(_reprojections(back) - before).max() < 1e-9
    moved.transform(T.inverse())
    assert np.allclose(moved._xyz[:moved._n], rec._xyz[:rec._n], atol=1e-12)


def test_shared_observation_vote():
    """A hand-made pair of models: three images with four 2D points each; the source has points 1, 2, 3, the target the
    points 1 .. 4, image "c" exists in the source only under another name."""
    def model(names, pids):
        rec = pc.Reconstruction()
        rec.add_camera(pc.Camera("SIMPLE_PINHOLE", 100, 100, [50.0, 50.0, 50.0], 0))
        n = max(max(p) for p in pids)
        rec.add_points3D(np.arange(3 * n, dtype=np.float64).reshape(n, 3))
        for i, (name, p) in enumerate(zip(names, pids)):
            im = pc.Image(i, name, 0, pc.Rigid3d())
            im.points2D = pc.ListPoint2D.from_arrays(np.zeros((len(p), 2)), np.array(p, np.int64))
            im._registered = True
            rec.add_image(im)
        return rec
    #                         image a          image b          image c / d
    src = model(["a", "b", "d"], [[1, 2, 3, -1], [1, 2, 3, 3], [1, 2, 3, -1]])
    tgt = model(["a", "b", "c"], [[2, 4, 1, 3], [2, 4, 3, 1], [1, 1, 1, 1]])
    # source 1 sees target 2 twice (a0, b0); source 2 sees target 4 twice; source 3 sees target 1 (a2), 3 (b2) and 1 (b3):
    # target 1 wins 2 : 1; image d has no namesake and votes for nothing
    ps, pt = pc.common_point_votes(src, tgt, min_common_observations=2)
    assert ps.tolist() == [1, 2, 3] and pt.tolist() == [2, 4, 1]
    assert pc.common_point_votes(src, tgt, min_common_observations=3)[0].tolist() == []
    # a tie goes to the smaller target id: without b3 source 3 sees targets 1 and 3 once each
    src2 = model(["a", "b", "d"], [[1, 2, 3, -1], [1, 2, 3, -1], [1, 2, 3, -1]])
    ps, pt = pc.common_point_votes(src2, tgt, min_common_observations=1)
    assert ps.tolist() == [1, 2, 3] and pt.tolist() == [2, 4, 1]
    assert pc.align_reconstructions_via_points(src, tgt, min_common_observations=3) is None      # nothing in common: no device touched
