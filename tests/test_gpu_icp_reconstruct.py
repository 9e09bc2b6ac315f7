"""Registration on the project's own dense model: the fused cloud and the mesh of tests/test_gpu_dense_metric.py's run (6 frames
of 48 x 64).  A copy of the cloud moved by a known small Sim(3) is registered back by GeometryRunner.register_dense_model,
against the cloud (its fused normals, point to plane: the truth is a zero of the cost, so it is recovered to rounding) and
against the mesh; evaluate_dense_model(transform=...) then measures the registered copy against the cloud at zero up to
rounding; the call sets only its own key.  Against the mesh there are two cases: points ON the mesh (the centroids of its
faces) moved by the known Sim(3), for which the truth is a zero of the cost and must be recovered; and the moved copy of the
cloud, which does not lie on the mesh, for which the fit is compared."""
import numpy as np
import pytest
import torch

from tests import icp_cases as C
from tests import test_gpu_dense_metric as TD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("icp_reconstruct")


def _moved_points(xyz, voxel):
    """xyz (N,3) numpy moved by the inverse of the known Sim(3) of _moved, about their centre"""
    centre = xyz.mean(0)
    s, R = 1.002, C.rotation([2.0, -1.0, 1.5], 0.2)
    t = centre - s * R @ centre + voxel * np.array([0.08, -0.05, 0.04])
    truth = (s, R, t)
    return torch.from_numpy(np.ascontiguousarray(C.apply(C.invert(truth), xyz))).cuda(), truth


def _moved(cloud, voxel):
    """the cloud's points moved by the inverse of a known Sim(3) about the cloud's centre: 0.2 degrees, 0.1 voxel, 0.2 %: a quarter of a voxel at
    the rim, well inside the spacing of the points"""
    xyz = cloud.xyz.cpu().numpy()
    centre = xyz.mean(0)
    s, R = 1.002, C.rotation([2.0, -1.0, 1.5], 0.2)
    t = centre - s * R @ centre + voxel * np.array([0.08, -0.05, 0.04])
    truth = (s, R, t)
    return torch.from_numpy(np.ascontiguousarray(C.apply(C.invert(truth), xyz))).cuda(), truth


def test_register_dense_model_recovers_a_known_sim3(tmp):
    runner, pred, mesh, cloud, voxel = TD._run(tmp)
    moved, truth = _moved(cloud, voxel)
    size = float(np.abs(cloud.xyz.cpu().numpy()).max())
    pred.pop("dense_registration", None)
    before = {k: v for k, v in pred.items()}
    start = dict(pred, fused_point_cloud=cloud._replace(xyz=moved))
    keys = set(start)
    out = runner.register_dense_model(start, cloud, 3.0 * voxel, estimate_scale=True, iterations=30)
    assert out is start and set(start) == keys | {"dense_registration"} and all(start[k] is v for k, v in before.items() if k != "fused_point_cloud")
    reg = start["dense_registration"]
    assert set(reg) == {"scale", "R", "t", "transform", "status", "iterations", "rmse", "fitness"}
    err = C.transform_error((reg["scale"], reg["R"].numpy(), reg["t"].numpy()), truth)
    print(f"\nagainst the cloud ({cloud.xyz.shape[0]} points, voxel {voxel:.4f}): {reg['status']} after {reg['iterations']}, "
          f"error {err:.2e}, rmse {reg['rmse']:.2e}, fitness {reg['fitness']:.4f}")
    assert reg["status"] == "converged" and err <= 1e-10 * max(size, 1.0) and reg["fitness"] == 1.0
    scale, R, t = reg["transform"]
    assert scale.is_cuda and R.is_cuda and t.is_cuda and float(scale) == reg["scale"]
    runner.evaluate_dense_model(start, cloud, [0.5 * voxel], 3.0 * voxel, transform=reg["transform"])
    m = start["dense_metrics"]
    print(f"accuracy after registration {m['accuracy']:.2e}, completeness {m['completeness']:.2e}, fscore {m['fscore']}")
    assert m["accuracy"] < 1e-9 and m["completeness"] < 1e-9 and m["fscore"] == [1.0]
    # without the registration the same evaluation is off by a fraction of a voxel
    runner.evaluate_dense_model(start, cloud, [0.5 * voxel], 3.0 * voxel)
    assert start["dense_metrics"]["accuracy"] > 0.05 * voxel


def test_register_dense_model_recovers_a_known_sim3_against_the_mesh(tmp):
    """Points that lie ON the mesh -- the centroid of every face with an area -- moved by the known Sim(3) and registered to
    the faces, point to plane: the truth is a zero of the cost (each centroid in the interior of its own face, away from the
    creases), so it is the minimum that Gauss-Newton reaches, and it is recovered to the accuracy that
    evaluate_dense_model's 1e-9 needs: 1e-9 x the size of the coordinates.  (The model's own VERTICES would sit on the
    creases of the distance function, every one of them, and the cloud does not lie on the mesh: see the next test.)"""
    runner, pred, mesh, cloud, voxel = TD._run(tmp)
    v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy().astype(np.int64)
    tri = v[f]
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    on_mesh = tri[area > 1e-6 * voxel * voxel].mean(1)
    assert len(on_mesh) > 0.9 * len(f)
    moved, truth = _moved_points(on_mesh, voxel)
    size = float(np.abs(v).max())
    start = dict(pred, dense_mesh=mesh._replace(vertices=moved))
    start.pop("dense_registration", None)
    keys = set(start)
    runner.register_dense_model(start, mesh, 3.0 * voxel, which="dense_mesh", estimate_scale=True, iterations=40)
    assert set(start) == keys | {"dense_registration"}
    reg = start["dense_registration"]
    err = C.transform_error((reg["scale"], reg["R"].numpy(), reg["t"].numpy()), truth)
    print(f"\n{len(on_mesh)} face centroids against the mesh ({len(f)} faces, voxel {voxel:.4f}): {reg['status']} after "
          f"{reg['iterations']}, error {err:.2e}, rmse {reg['rmse']:.2e}, fitness {reg['fitness']:.4f}")
    assert reg["status"] == "converged" and err <= 1e-9 * max(size, 1.0) and reg["rmse"] <= 1e-9 * max(size, 1.0) and reg["fitness"] == 1.0


def test_register_dense_model_against_the_mesh(tmp):
    """The moved copy of the cloud registered to the MESH of the same depth maps.  The cloud does not lie on the mesh (the two
    differ by the noise of the maps and the voxel size), so the minimum of the cost is not the truth and the scene, close to
    a plane, lets the pose slide along it: the transform is recovered in the test above, on points that lie on the mesh.  What
    must hold here: the run converges, the pose found fits the mesh at least as well as the true pose does (the cost that ICP
    descends, measured by icp_step at both), and better than the start; no pair is lost."""
    from vggsfm_amd import registration

    runner, pred, mesh, cloud, voxel = TD._run(tmp)
    moved, truth = _moved(cloud, voxel)
    max_dist = 3.0 * voxel
    target = registration.make_target(mesh, max_dist)
    as_torch = lambda T: (float(T[0]), torch.from_numpy(np.ascontiguousarray(T[1])), torch.from_numpy(np.ascontiguousarray(T[2])))
    rms = lambda step: float(np.sqrt(step.sq_error / step.count))
    at_truth = registration.icp_step(moved, target, as_torch(truth), max_dist, estimate_scale=True)
    at_start = registration.icp_step(moved, target, None, max_dist, estimate_scale=True)
    start = dict(pred, fused_point_cloud=cloud._replace(xyz=moved))
    keys = set(start)
    runner.register_dense_model(start, target, max_dist, estimate_scale=True, iterations=40, rotation_tol=1e-7,
                                translation_tol=1e-7 * voxel, scale_tol=1e-7)
    assert set(start) == keys | {"dense_registration"}
    reg = start["dense_registration"]
    found = registration.icp_step(moved, target, (reg["scale"], reg["R"], reg["t"]), max_dist, estimate_scale=True)
    err = C.transform_error((reg["scale"], reg["R"].numpy(), reg["t"].numpy()), truth)
    print(f"\nagainst the mesh ({mesh.faces.shape[0]} faces): {reg['status']} after {reg['iterations']}; rms distance to the faces "
          f"{rms(at_start):.3e} at the start, {rms(at_truth):.3e} at the truth, {rms(found):.3e} found (voxel {voxel:.4f}); "
          f"difference to the truth {err:.2e}; pairs {at_truth.count} / {found.count}")
    assert reg["status"] == "converged" and 1 <= reg["iterations"] < 40
    assert rms(found) <= rms(at_truth) < rms(at_start) and found.count >= at_truth.count
    assert abs(reg["rmse"] - rms(found)) <= 1e-12 and reg["fitness"] == found.count / moved.shape[0]
    with pytest.raises(ValueError, match="which must be"):
        runner.register_dense_model(dict(pred), mesh, voxel, which="depth_dict")
