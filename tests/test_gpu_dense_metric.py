"""The dense metrics on the project's own dense model: GeometryRunner.dense_reconstruct_from_frames(patchmatch_iterations=4),
the fusion, then mesh_dense_surface(resolution=40), on the reconstruction of tests/test_gpu_mvs_reconstruct.py (6 frames of
48 x 64).  The distances of the fused points to the mesh equal the all-pairs restatement of tests/nearest_cases.py on the
read-back data bit for bit; a point is never farther from the mesh than from the nearest vertex of a face (true of any
mesh: it ties the triangle kernel to the point kernel); a cloud against itself and against a shifted copy gives what it must."""
import functools

import numpy as np
import pytest
import torch

from tests import nearest_cases as C
from tests import test_gpu_meshing_reconstruct as TM

pytestmark = pytest.mark.gpu

POINTS = 1500


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("dense_metric")


@functools.lru_cache(maxsize=None)
def _run(tmp):
    sc, rec, images, runner, pred, _, _ = TM._run(tmp)
    pred = runner.fuse_dense_point_cloud(pred, images)
    mesh, cloud = pred["dense_mesh"], pred["fused_point_cloud"]
    v = mesh.vertices.cpu().numpy()
    voxel = float((v.max(0) - v.min(0)).max()) / TM.RESOLUTION               # about the volume's voxel
    return runner, pred, mesh, cloud, voxel


def test_cloud_to_mesh_is_the_restatement_and_never_beyond_the_nearest_vertex(tmp):
    from vggsfm_amd import nearest
    from vggsfm_amd.utils import dense_metric

    _, _, mesh, cloud, voxel = _run(tmp)
    pts = cloud.xyz[:POINTS].contiguous()
    assert pts.shape[0] == POINTS and mesh.faces.shape[0] > 500
    max_dist, taus = 3.0 * voxel, [0.25 * voxel, voxel]
    metrics, got = dense_metric.cloud_to_mesh(pts, mesh, taus, max_dist, return_distances=True)
    v, f, p = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), pts.cpu().numpy()
    ref = C.nearest_face(v, f, p, max_dist)
    face, dist2, closest = got.face.cpu().numpy(), got.dist2.cpu().numpy(), got.closest.cpu().numpy()
    assert face.tobytes() == ref["face"].tobytes() and dist2.tobytes() == ref["dist2"].tobytes()
    assert np.array_equal(np.isnan(closest), np.isnan(ref["closest"])) and \
        np.nan_to_num(closest).tobytes() == np.nan_to_num(ref["closest"]).tobytes()
    # the metrics' counts are the restatement's, exactly
    found, below, sum_d, sum_d2 = C.distance_stats(ref["dist2"], taus)
    back = C.nearest_point(p, v, max_dist)
    found_g, below_g, _, _ = C.distance_stats(back["dist2"], taus)
    assert (metrics["num_pred"], metrics["found_pred"], metrics["num_gt"], metrics["found_gt"]) == (POINTS, found, len(v), found_g)
    assert metrics["precision"] == [b / POINTS for b in below] and metrics["recall"] == [b / len(v) for b in below_g]
    assert abs(metrics["accuracy"] * found - sum_d) <= POINTS * 2.0 ** -52 * sum_d
    # to the mesh <= to its nearest vertex, for every point (both searched within the same radius).  "Vertex" means a vertex
    # of a face: this mesh has 6 vertices that no face names (3 699 vertices, 7 002 faces; the extraction emits them and the
    # meshing is not this change's to alter), and a surface is no nearer to a point for a vertex it does not contain.
    on_surface = torch.unique(mesh.faces.long())
    assert 0 <= mesh.vertices.shape[0] - on_surface.shape[0] < 0.01 * mesh.vertices.shape[0]
    to_vertex = nearest.nearest_points(mesh.vertices[on_surface], pts, max_dist).distance.cpu().numpy()
    to_mesh = np.sqrt(dist2)
    assert (to_mesh <= to_vertex * (1.0 + 1e-12)).all()
    both = np.isfinite(to_vertex)
    print(f"\n{POINTS} fused points against {len(f)} faces / {len(v)} vertices, voxel ~ {voxel:.4f}: found {found}, accuracy "
          f"{metrics['accuracy']:.5f}, mean to the nearest vertex {to_vertex[both].mean():.5f}; precision {metrics['precision']}, "
          f"recall {metrics['recall']}, fscore {metrics['fscore']}; gaps {ref['gap_best']:.2e} {ref['gap_r2']:.2e}")
    assert found > 0.9 * POINTS and (to_mesh[both] < to_vertex[both]).mean() > 0.5


def test_a_cloud_against_itself_and_against_a_shifted_copy(tmp):
    from vggsfm_amd.utils import dense_metric

    _, _, _, cloud, voxel = _run(tmp)
    xyz = cloud.xyz
    n = xyz.shape[0]
    taus, max_dist = [0.5 * voxel, 2.0 * voxel], 4.0 * voxel
    same = dense_metric.evaluate_dense(cloud, xyz, taus, max_dist)
    assert same["accuracy"] == 0.0 and same["completeness"] == 0.0 and same["overall_rms"] == 0.0
    assert same["fscore"] == [1.0, 1.0] and same["found_pred"] == same["found_gt"] == same["num_pred"] == same["num_gt"] == n
    s = 1.25 * voxel
    shifted = xyz + torch.tensor([s, 0.0, 0.0], dtype=torch.float64, device=xyz.device)
    moved = dense_metric.cloud_to_cloud(shifted, cloud, taus, max_dist)
    # the copy's own original is a candidate at distance s (to the rounding of the shift), so no nearest distance exceeds it
    assert moved["found_pred"] == n and 0.0 < moved["accuracy"] <= s * (1.0 + 1e-12) and moved["completeness"] <= s * (1.0 + 1e-12)
    assert moved["precision"][1] == 1.0 and moved["recall"][1] == 1.0 and moved["fscore"][1] == 1.0
    # the same through a Sim(3) that undoes the shift: back to zero up to the rounding of the transform
    eye = torch.eye(3, dtype=torch.float64, device=xyz.device)
    undone = dense_metric.evaluate_dense(shifted, cloud, taus, max_dist,
                                         transform=(1.0, eye, torch.tensor([-s, 0.0, 0.0], dtype=torch.float64, device=xyz.device)))
    assert undone["accuracy"] < 1e-12 and undone["fscore"] == [1.0, 1.0]


def test_evaluate_dense_model_sets_one_key(tmp):
    from vggsfm_amd.utils import dense_metric

    runner, pred, mesh, cloud, voxel = _run(tmp)
    pred.pop("dense_metrics", None)
    before = {k: v for k, v in pred.items()}
    taus, max_dist = [voxel], 3.0 * voxel
    out = runner.evaluate_dense_model(pred, mesh, taus, max_dist)
    assert out is pred and set(pred) == set(before) | {"dense_metrics"} and all(pred[k] is before[k] for k in before)
    assert pred["dense_metrics"] == dense_metric.evaluate_dense(cloud, mesh, taus, max_dist)
    m = pred["dense_metrics"]
    assert m["num_pred"] == cloud.xyz.shape[0] and m["num_gt"] == mesh.vertices.shape[0] and 0.0 < m["fscore"][0] <= 1.0
    runner.evaluate_dense_model(pred, cloud.xyz, taus, max_dist, which="dense_mesh")
    m2 = pred["dense_metrics"]
    assert m2["num_pred"] == mesh.vertices.shape[0] and m2["num_gt"] == cloud.xyz.shape[0]
    assert (m2["found_gt"], m2["recall"]) == (m["found_pred"], m["precision"])       # the same direction, measured from the other side
    with pytest.raises(ValueError, match="which must be"):
        runner.evaluate_dense_model(pred, mesh, taus, max_dist, which="depth_dict")
    print(f"\nfused cloud against the mesh of the same maps: {m}")
