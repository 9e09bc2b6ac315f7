"""Frames and a sparse reconstruction in, ONE triangle mesh out, with no learned part:
GeometryRunner.dense_reconstruct_from_frames(patchmatch_iterations=4), then GeometryRunner.mesh_dense_surface, on the
reconstruction of tests/test_gpu_mvs_reconstruct.py -- 6 frames of 48 x 64 under one SIMPLE_RADIAL camera (k = 0.08) in front
of the slanted plane of tests/mvs_cases.py, 24 planes, a grid of 40 nodes along the longest side of the maps' points, every
other option at its default (margin 0.05, truncation 4 voxels, min_weight 1, unit weights).

The mesh must equal, bit for bit, the NumPy restatement of tests/meshing_cases.py applied to the depth maps and frames read
back from the device, on the grid that volume_bounds gave: no tolerance and no CPU stereo.  The distance of the vertices from
the true plane is that of the stereo's depth maps averaged over the views, not of the meshing; it is asserted at 2 x what
the restatement measures on the same maps, computed on the CPU in this test.  As conditions on the restatement alone: at
least a quarter of the nodes are valid and there are faces."""
import functools

import numpy as np
import pytest
import torch

from tests import fusion_cases as FC
from tests import meshing_cases as C
from tests import mvs_cases as MC
from vggsfm_amd import dense_depth as DD
from vggsfm_amd import meshing
from vggsfm_amd.runners import GeometryConfig, GeometryRunner
from vggsfm_amd.utils.tensor_to_pycolmap import batch_matrix_to_pycolmap

pytestmark = pytest.mark.gpu

PLANES, ITERATIONS, RESOLUTION = 24, 4, 40


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
    images = torch.from_numpy(FC.colours(sc["frames"])).cuda()[None].contiguous()            # (1,S,3,H,W) colours
    runner = GeometryRunner(GeometryConfig())
    pred = runner.dense_reconstruct_from_frames({"reconstruction": rec}, images, num_planes=PLANES, patchmatch_iterations=ITERATIONS)
    before = {k: v for k, v in pred.items()}
    path = str(tmp / "mesh.ply")
    pred = runner.mesh_dense_surface(pred, images, output_path=path, resolution=RESOLUTION)
    return sc, rec, images, runner, pred, before, path


@functools.lru_cache(maxsize=None)
def _restated(tmp):
    """the restatement on what the device holds: depth maps and frames read back, the grid of volume_bounds"""
    sc, rec, images, _, pred, _, _ = _run(tmp)
    ids = sorted(int(i) for i in rec.reg_image_ids())
    depth = np.stack([pred["depth_dict"][rec.images[i].name].cpu().numpy() for i in ids])
    pose, cam = DD._camera_rows(rec, ids)
    dev = images.device
    origin, voxel, dims = meshing.volume_bounds(
        meshing._depth_points(torch.from_numpy(depth).to(dev), torch.from_numpy(pose).to(dev), torch.from_numpy(cam).to(dev), 4),
        RESOLUTION, 0.05)
    frames = images[0].cpu().numpy()[ids]
    trunc = 4.0 * voxel
    vols = C.integrate(depth, None, frames, pose, cam, origin, voxel, dims, trunc, *C.empty_volume(dims))
    ref = C.extract(vols[0], vols[1], vols[2], origin, voxel, dims, 1.0)
    ref["weight_sum"] = vols[1]
    conf = np.stack([pred["depth_conf_dict"][rec.images[i].name].cpu().numpy() for i in ids])
    return ids, depth, conf, (origin, voxel, dims), ref, dict(vols[3], **ref["margins"])


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("meshing")


def test_mesh_is_the_restatement_on_the_read_back_maps(tmp):
    _, _, _, _, pred, before, _ = _run(tmp)
    _, depth, _, (origin, voxel, dims), ref, margins = _restated(tmp)
    mesh = pred["dense_mesh"]
    assert isinstance(mesh, meshing.Mesh) and all(t.is_cuda for t in mesh)
    assert set(pred) == set(before) | {"dense_mesh"} and all(pred[k] is before[k] for k in before)        # no other key changes
    got = meshing.Mesh(*(t.cpu().numpy() for t in mesh))
    valid = float((ref["weight_sum"] >= 1.0).mean())
    print(f"\ngrid {dims} at voxel {voxel:.4f} from {origin}: {len(got.vertices)} vertices, {len(got.faces)} faces (restatement "
          f"{len(ref['vertices'])}, {len(ref['faces'])}); valid nodes {valid:.3f}; margins { {k: f'{v:.1e}' for k, v in margins.items()} }")
    assert valid >= 0.25 and len(ref["faces"]) > 0                           # conditions on the restatement alone
    assert max(dims) == RESOLUTION
    assert got.vertices.shape == ref["vertices"].shape and got.faces.shape == ref["faces"].shape
    for k in ("vertices", "rgb", "faces", "normals"):
        assert getattr(got, k).tobytes() == ref[k].tobytes(), (k, int((getattr(got, k) != ref[k]).sum()))


def test_distance_to_the_true_plane_and_orientation(tmp):
    """At 2 x what the restatement gives on the same read-back maps (CPU), never against the kernel's own output; every
    face's geometric normal points to the half-space of every camera's centre (and, the cameras looking along +z, has a
    negative z).  Measured (one MI355X): grid 40 x 32 x 13 at voxel 0.0855, 3 699 vertices, 7 002 faces, 58.7 % of the nodes
    valid; distance to the plane 2.24e-3 in the median, 5.09e-2 at most (the restatement's: the same); all 7 002 faces look
    at all six cameras."""
    _, _, _, _, pred, _, _ = _run(tmp)
    ref = _restated(tmp)[4]
    mesh = pred["dense_mesh"]
    want = FC.plane_distance(ref["vertices"])
    vertices, faces = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    got = FC.plane_distance(vertices)
    n, c = C.face_normals(vertices, faces)
    print(f"\ndistance to the plane: median {np.median(got):.4e}, largest {got.max():.4e} (restatement: {np.median(want):.4e}, "
          f"{want.max():.4e})")
    assert got.max() <= 2 * want.max() and np.median(got) <= 2 * np.median(want)
    sc = MC.reconstruction_scene()
    centres = np.stack([-p[:, :3].T @ p[:, 3] for p in sc["poses"]])
    facing = [int(((n * (centre - c)).sum(-1) > 0).sum()) for centre in centres]
    print(f"faces that look at each camera, of {len(faces)}: {facing}; with a negative z of the normal: {int((n[:, 2] < 0).sum())}")
    assert facing == [len(faces)] * len(centres) and (n[:, 2] < 0).all()    # every face looks at every camera
    assert faces.min() >= 0 and faces.max() < len(vertices) and np.isfinite(vertices).all()
    assert np.isfinite(mesh.normals.cpu().numpy()).all() and np.isfinite(mesh.rgb.cpu().numpy()).all()


def test_options_bounds_weights_and_refusals(tmp):
    _, rec, images, runner, pred, _, _ = _run(tmp)
    ids, depth, conf, bounds, ref, _ = _restated(tmp)
    start = {"reconstruction": rec, "depth_dict": pred["depth_dict"], "depth_conf_dict": pred["depth_conf_dict"]}
    mesh = pred["dense_mesh"]
    given = runner.mesh_dense_surface(dict(start), images, bounds=bounds)["dense_mesh"]             # the same grid, given
    for a, b in zip(mesh, given):
        assert torch.equal(a, b)
    plain = runner.mesh_dense_surface(dict(start), None, bounds=bounds)["dense_mesh"]               # colours are optional
    assert torch.equal(plain.vertices, mesh.vertices) and torch.equal(plain.faces, mesh.faces) and not plain.rgb.any()
    # the confidences as weights: the restatement with the read-back confidences, bit for bit
    pose, cam = DD._camera_rows(rec, ids)
    origin, voxel, dims = bounds
    frames = images[0].cpu().numpy()[ids]
    vols = C.integrate(depth, conf, frames, pose, cam, origin, voxel, dims, 4.0 * voxel, *C.empty_volume(dims))
    want = C.extract(vols[0], vols[1], vols[2], origin, voxel, dims, 0.5)
    weighted = runner.mesh_dense_surface(dict(start), images, confidence_weights=True, bounds=bounds, min_weight=0.5)["dense_mesh"]
    assert len(want["faces"]) > 0
    for k in ("vertices", "rgb", "faces", "normals"):
        assert getattr(weighted, k).cpu().numpy().tobytes() == want[k].tobytes(), k
    with pytest.raises(ValueError, match="images must be"):
        runner.mesh_dense_surface(dict(start), images[..., :-1].contiguous())
    with pytest.raises(ValueError, match="has no frame"):
        runner.mesh_dense_surface(dict(start), images[:, :-1].contiguous())
    with pytest.raises(ValueError, match="min_weight"):
        runner.mesh_dense_surface(dict(start), images, bounds=bounds, min_weight=0.0)
    with pytest.raises(ValueError, match="resolution"):
        runner.mesh_dense_surface(dict(start), images, resolution=1)
    with pytest.raises(ValueError, match="nothing to mesh"):
        runner.mesh_dense_surface({"reconstruction": rec, "depth_dict": {}}, images)


def test_ply_reads_back_to_the_mesh(tmp):
    _, _, _, _, pred, _, path = _run(tmp)
    mesh = pred["dense_mesh"]
    back = meshing.read_mesh_ply(path)
    assert back.vertices.tobytes() == mesh.vertices.cpu().numpy().tobytes()
    assert back.normals.tobytes() == mesh.normals.cpu().numpy().tobytes()
    assert back.faces.tobytes() == mesh.faces.cpu().numpy().tobytes()
    assert np.abs(back.rgb.astype(np.float64) - np.clip(mesh.rgb.cpu().numpy(), 0, 1)).max() <= 0.5 / 255 + 1e-7
