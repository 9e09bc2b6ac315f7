"""Host-side logic of the dense depth stage (vggsfm_amd/dense_depth.py): the reference's key and observation order, packing
of ragged maps and recorded draws, argument validation, and the (N,3) transforms of the compat objects it relies on."""
import numpy as np
import pytest
import torch

from vggsfm_amd import dense_depth as DD
from vggsfm_amd import pycolmap_compat as pc
from vggsfm_amd.scene import make_scene


def _reference_loop_order(rec):
    """runner.py:757-770 restated on the compat object: keys in order of first appearance, (point id, image) rows."""
    order = {}
    for pid in rec.points3D:
        for el in rec.points3D[pid].track.elements:
            order.setdefault(rec.images[el.image_id].name, []).append(pid)
    return order


@pytest.mark.parametrize("shared", [False, True])
def test_sparse_order_is_the_reference_loop_order(shared):
    sc = make_scene(7, 120, "SIMPLE_RADIAL", shared_camera=shared, seed=4)
    rec = pc.Reconstruction.from_arrays(sc.points3D, sc.extrinsics, sc.intrinsics, sc.tracks, sc.mask,
                                        np.array([1024, 1024]), shared_camera=shared, camera_type="SIMPLE_RADIAL",
                                        extra_params=sc.extra_params)
    rec.delete_point3D(1)                                   # dead rows and an image whose first point went away
    rec.delete_point3D(5)
    image_ids, prow, slot, pid, obs_ptr = DD.sparse_order(rec)
    ref = _reference_loop_order(rec)
    assert [rec.images[i].name for i in image_ids] == list(ref)
    assert obs_ptr[-1] == len(pid) == len(prow) == len(slot)
    for k, name in enumerate(ref):
        a, b = obs_ptr[k], obs_ptr[k + 1]
        assert pid[a:b].tolist() == ref[name]
        assert (slot[a:b] == k).all()
    assert np.array_equal(prow, pid - 1)


def test_sparse_order_of_an_empty_model():
    rec = pc.Reconstruction()
    image_ids, prow, slot, pid, obs_ptr = DD.sparse_order(rec)
    assert image_ids == [] and len(pid) == 0 and obs_ptr.tolist() == [0]


def test_camera_rows_pinhole_has_zero_k():
    sc = make_scene(3, 50, "SIMPLE_PINHOLE", seed=2)
    rec = pc.Reconstruction.from_arrays(sc.points3D, sc.extrinsics, sc.intrinsics, sc.tracks, sc.mask,
                                        np.array([1024, 1024]))
    pose, cam = DD._camera_rows(rec, [2, 0])
    assert np.array_equal(pose[0], sc.extrinsics[2]) and np.array_equal(pose[1], sc.extrinsics[0])
    assert np.array_equal(cam[:, 3], [0.0, 0.0]) and cam[0, 0] == sc.intrinsics[2, 0, 0]


def test_pack_maps_offsets_and_validation():
    maps = [np.arange(6, dtype=np.float32).reshape(2, 3), torch.ones((4, 1), dtype=torch.float32),
            np.zeros((3, 5), np.float32)]
    p = DD.pack_maps(maps, device="cpu")
    assert p.off.tolist() == [0, 6, 10, 25] and p.heights.tolist() == [2, 4, 3] and p.widths.tolist() == [3, 1, 5]
    assert p.max_pixels == 15 and p.flat.dtype == torch.float32
    assert p.flat[:6].tolist() == list(range(6))
    with pytest.raises(ValueError, match="float32"):
        DD.pack_maps([np.zeros((2, 2))], device="cpu")
    with pytest.raises(ValueError, match="2-D"):
        DD.pack_maps([np.zeros((2, 2, 1), np.float32)], device="cpu")


def test_pack_samples():
    d = DD.pack_samples([np.array([[0, 1], [2, 3]]), np.zeros((0, 2)), [[5, 4]]], 3)
    assert d.shape == (3, 2, 2) and d.dtype == np.int32
    assert d[0].tolist() == [[0, 1], [2, 3]] and (d[1] == -1).all() and d[2].tolist() == [[5, 4], [-1, -1]]
    with pytest.raises(ValueError):
        DD.pack_samples([np.zeros((1, 2))], 2)
    with pytest.raises(ValueError):
        DD.pack_samples([np.array([[-3, 1]])], 1)


def test_status_errors():
    with pytest.raises(ValueError, match="Too few points for depth alignment"):
        DD.raise_for_status(1)
    with pytest.raises(ValueError, match="Ill-posed scene for depth alignment"):
        DD.raise_for_status(2)
    with pytest.raises(ValueError, match="consensus"):
        DD.raise_for_status(3)
    DD.raise_for_status(0)


def test_compat_transforms_take_point_arrays():
    rng = np.random.default_rng(0)
    R = pc.Rotation3d(np.array([0.1, -0.2, 0.3, 0.9]))
    T = pc.Rigid3d(R, rng.normal(size=3))
    P = rng.normal(size=(5, 3))
    np.testing.assert_allclose(T * P, np.stack([T * p for p in P]), rtol=1e-15, atol=1e-15)
    np.testing.assert_allclose(T.inverse() * (T * P), P, atol=1e-12)
    np.testing.assert_allclose(R * P, np.stack([R * p for p in P]), rtol=1e-15, atol=1e-15)
