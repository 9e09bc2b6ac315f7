"""Masked multi-view triangulation, the part that needs no GPU: a numpy restatement of every function against every golden
on the admitted set (bounds: tests/multiview_cases.py), the admission caps on the committed files, the host-only entry logic
and the error paths."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import multiview_cases as MC
from vggsfm_amd import _lib
from vggsfm_amd.utils import triangulation as TR
from vggsfm_amd.utils import triangulation_helpers as TH



def test_every_golden_file_is_known_and_small():
    assert sorted(os.path.basename(f) for f in MC.files()) == sorted(f"multiview_{n}.npz" for n in MC.ALL_FILES)
    assert all(os.path.getsize(f) < 1_000_000 for f in MC.files())


@pytest.mark.parametrize("name", MC.TRI_CASES + MC.LR_CASES + ("from_tracks",))
def test_admission_caps_hold(name):
    g = MC.load(name)
    for key in ("admit_points", "admit_che", "admit_flag"):
        if key in g:
            assert 1.0 - g[key].mean() <= MC.CAP, f"{name}: {key} leaves out more than {MC.CAP:.0%}"
            assert g[key].dtype == np.bool_
    # an angle is left out only with its point
    assert g["ref_points"].dtype == np.float64


@pytest.mark.parametrize("name", MC.TRI_CASES)
def test_numpy_restatement_of_the_solve_equals_the_reference(name):
    g = MC.load(name)
    ext, tracks = g["extrinsics"], g["tracks"].astype(np.float64)
    S, N = tracks.shape[:2]
    cams = np.broadcast_to(ext, (N, S, 3, 4))
    mask = g["mask"].T if "mask" in g else None
    X, invalid = MC.np_triangulate(cams, tracks.transpose(1, 0, 2), mask)
    table = MC.np_angle_table(cams, X)
    da, dc = MC.angle_deviation(table, g["ref_angles"], g["admit_points"][:, None])
    MC.assert_close(f"numpy {name}", {"points": MC.point_deviation(X, g["ref_points"], g["admit_points"]), "angles": da,
                                      "cosines": dc})
    assert (invalid == g["ref_invalid"])[g["admit_che"]].all()
    assert ((table.max(1) >= g["min_tri_angle"]) == (g["ref_angles"].max(1) >= g["min_tri_angle"]))[g["admit_flag"]].all()


def test_numpy_restatement_from_tracks():
    g = MC.load("from_tracks")
    S, N = g["tracks"].shape[1:3]
    X, invalid = MC.np_triangulate(np.broadcast_to(g["extrinsics"][0], (N, S, 3, 4)), g["tracks"][0].transpose(1, 0, 2),
                                   g["mask"][0].T)
    MC.assert_close("numpy from_tracks", {"points": MC.point_deviation(X, g["ref_points"][0], g["admit_points"][0])})
    assert (~invalid == g["ref_cheirality"][0])[g["admit_che"][0]].all()


@pytest.mark.parametrize("name", MC.LR_CASES)
def test_numpy_restatement_of_local_refinement(name):
    g = MC.load(name)
    X, flag, invalid = MC.np_local_refinement(g["points1"], g["extrinsics"], float(g["min_tri_angle"]), g["inlier_mask"],
                                              g["sorted_indices"], int(g["lo_num"]))
    MC.assert_close(f"numpy {name}", {"points": MC.point_deviation(X, g["ref_points"], g["admit_points"])})
    assert (flag == g["ref_tri_angle_masks"])[g["admit_flag"]].all()
    assert (invalid == g["ref_invalid"])[g["admit_che"]].all()


def test_numpy_restatement_of_the_angle_functions():
    g = MC.load("angles")
    for what, got, ref in (("batched", MC.np_angle_table(g["batched_extrinsics"], g["batched_points"], float(g["batched_eps"])),
                            g["ref_batched"]),
                           ("exhaustive", MC.np_angle_exhaustive(g["exhaustive_extrinsics"], g["exhaustive_points"]),
                            g["ref_exhaustive"]),
                           ("pairs", MC.np_angle_pairs(g["pairs_center1"], g["pairs_center2"], g["pairs_points"],
                                                       float(g["pairs_eps"])), g["ref_pairs"])):
        assert got.shape == ref.shape
        da, dc = MC.angle_deviation(got, ref)
        MC.assert_close(f"numpy angles {what}", {"angles": da, "cosines": dc})
        i, j = MC.EPS_BRANCH[what]                                 # the eps branch: exactly 0 in both
        assert got[i, j] == 0.0 and ref[i, j] == 0.0


def test_numpy_restatement_of_the_angular_error():
    g = MC.load("angerr")
    for deg in (False, True):
        a, c = MC.np_angular_error(g["point2D"], g["point3D"], g["cam_from_world"], deg)
        ref = g["ref_deg"] if deg else g["ref_rad"]
        da, dc = MC.angle_deviation(a, ref, unit=np.pi / 180.0 if deg else 1.0, ref_cos=g["ref_cos"], got_cos=c)
        # (degrees are held to the bound in degrees, radians to the same number in radians: the tighter of the two)
        MC.assert_close(f"numpy angerr deg={deg}", {"angles": da, "cosines": dc})
        assert c.max() <= 1.0 and a.shape == (4, 6, 50)


def test_host_only_entry_logic():
    """What the entries decide on the host, before any launch: sizes and refusals (no GPU is touched)."""
    L = _lib.lib()
    assert L.vggx_multiview_workspace_bytes(1, 200) == 200 * 24 and L.vggx_multiview_workspace_bytes(3, 5) == 3 * 5 * 24
    assert L.vggx_multiview_workspace_bytes(2 ** 33, 2) == 2 ** 33 * 48            # a long arrives whole
    assert L.vggx_multiview_workspace_bytes(0, 5) == 0
    bad = -1
    # S < 1; angle mode without its outputs; an odd stride; cameras that do not cover the problems; n == 0 is a no-op
    assert L.vggx_multiview_triangulate(None, 1, 1, None, 1, 2, 2, None, 0, 0, 0, None, 4, 0, 0, 0, 0.0, None, None, None, None,
                                        None, None) == bad
    assert L.vggx_multiview_triangulate(None, 1, 1, None, 1, 2, 2, None, 0, 0, 0, None, 4, 3, 0, 1, 0.0, None, None, None, None,
                                        None, None) == bad
    assert L.vggx_multiview_triangulate(None, 1, 1, None, 1, 2, 2, None, 0, 0, 0, None, 0, 3, 0, 0, 0.0, None, None, None, None,
                                        None, None) == 0
    one = torch.zeros(64, dtype=torch.float64)
    assert L.vggx_multiview_triangulate(one, 1, 1, one, 1, 3, 2, None, 0, 0, 0, None, 4, 3, 0, 0, 0.0, one, None, None, None,
                                        None, None) == bad
    assert L.vggx_multiview_triangulate(one, 2, 1, one, 1, 2, 2, None, 0, 0, 0, None, 4, 3, 0, 0, 0.0, one, None, None, None,
                                        None, None) == bad
    assert L.vggx_max_tri_angle(one, 1, 1, one, 4, 3, 0, 0.0, one, None, one, None) == bad
    assert L.vggx_tri_angle_table(one, 2, one, 3, 2, 1e-12, one, one, None) == bad
    assert L.vggx_tri_angle_pairs(None, None, -1, None, 1, 1e-12, None, None) == bad
    assert L.vggx_angular_error(None, None, None, 0, 5, 5, 0, None, None, None) == 0
    assert L.vggx_view_centers(None, 3, None, None) == bad
    with pytest.raises(ctypes.ArgumentError):
        L.vggx_multiview_workspace_bytes(1, 2 ** 31)


# --- error paths of the public functions ------------------------------------------------------------------------------
def _cpu_scene(S=4, N=5):
    g = torch.Generator().manual_seed(0)
    ext = torch.eye(3, 4, dtype=torch.float64)[None].repeat(S, 1, 1)
    ext[:, 0, 3] = torch.arange(S, dtype=torch.float64)
    return ext, torch.rand(S, N, 2, generator=g, dtype=torch.float64)


def test_tensors_off_the_gpu_are_refused():
    ext, tracks = _cpu_scene()
    S, N = tracks.shape[:2]
    pts = torch.rand(N, 3, dtype=torch.float64)
    calls = [
        lambda: TR.triangulate_tracks_masked(ext, tracks),
        lambda: TR.max_triangulation_angle(ext, pts),
        lambda: TR.triangulate_multi_view_point_from_tracks(ext[None], tracks[None]),
        lambda: TH.triangulate_multi_view_point_batched(ext[None].expand(N, -1, -1, -1), tracks.permute(1, 0, 2)),
        lambda: TH.calculate_triangulation_angle_batched(ext[None].expand(N, -1, -1, -1), pts),
        lambda: TH.calculate_triangulation_angle_exhaustive(ext, pts),
        lambda: TH.calculate_triangulation_angle(pts, pts, pts),
        lambda: TH.calculate_normalized_angular_error_batched(tracks, pts[None].expand(2, -1, -1), ext),
        lambda: TH.local_refinement_tri(tracks.permute(1, 0, 2), ext[None].expand(N, -1, -1, -1), 1.5,
                                        torch.ones(N, 3, S, dtype=torch.bool), torch.zeros(N, 3, dtype=torch.long), lo_num=2),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_shape_asserts():
    ext, tracks = _cpu_scene()
    S, N = tracks.shape[:2]
    with pytest.raises(AssertionError, match="number of cameras and points"):
        TH.triangulate_multi_view_point_batched(ext[None].expand(N, -1, -1, -1)[:, :3], tracks.permute(1, 0, 2))
    with pytest.raises(AssertionError):
        TH.calculate_triangulation_angle_batched(ext[None].expand(N, -1, -1, -1), torch.zeros(N + 1, 3))
    with pytest.raises(AssertionError):
        TH.calculate_normalized_angular_error_batched(tracks, torch.zeros(2, N, 3), ext[:3])
    with pytest.raises(AssertionError):
        TR.triangulate_tracks_masked(ext, tracks, torch.ones(S, N + 1, dtype=torch.bool))
    with pytest.raises(AssertionError):
        TR.triangulate_tracks_masked(ext[:3], tracks)
    with pytest.raises(AssertionError):                               # fewer hypotheses than lo_num
        TH.local_refinement_tri(tracks.permute(1, 0, 2), ext[None].expand(N, -1, -1, -1), 1.5,
                                torch.ones(N, 3, S, dtype=torch.bool), torch.zeros(N, 3, dtype=torch.long), lo_num=50)


def test_size_guard_names_the_lean_function():
    """100,000 tracks x 200 views would be a 32 GB table: refused before anything is allocated or moved (the inputs here are
    expanded views of a few bytes)."""
    B, S = 100000, 200
    cams = torch.zeros(1, 1, 3, 4, dtype=torch.float64).expand(B, S, -1, -1)
    pts2 = torch.zeros(1, 1, 2, dtype=torch.float64).expand(B, S, -1)
    X = torch.zeros(1, 3, dtype=torch.float64).expand(B, -1)
    assert 8 * B * S * S > TH.MAX_ANGLE_TABLE_BYTES == 2 ** 31
    for call in (lambda: TH.triangulate_multi_view_point_batched(cams, pts2, compute_tri_angle=True),
                 lambda: TH.calculate_triangulation_angle_batched(cams, X),
                 lambda: TH.calculate_triangulation_angle_exhaustive(cams[0], X),
                 lambda: TH.calculate_triangulation_angle(X, X, X)):
        with pytest.raises(ValueError, match="triangulate_tracks_masked"):
            call()
    with pytest.raises(RuntimeError, match="no CPU path"):            # without the table the size is no obstacle
        TH.triangulate_multi_view_point_batched(cams, pts2)
