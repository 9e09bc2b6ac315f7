"""CPU: the numpy oracle (oracle/geometry.py) against the REFERENCE's own torch functions on freshly seeded inputs -- shapes
and seeds that no golden vector of tests/test_oracle_golden.py has seen -- for every function of the torch half of the
path: project_3D_points, cam_from_img (undistortion), filter_all_points3D, triangulate_by_pair and triangulate_tracks
(LO-RANSAC; the torch.randperm draws the reference makes are recorded and replayed).  The reference's results are the
recorded calls of tests/golden/reference_calls/oracle_live_vs_reference.npz (oracle/ref_replay.py: re-recorded by running
this module with VGG_RECORD_REFERENCE=1 where the reference tree exists).  Same comparisons and tolerances as
tests/test_oracle_golden.py; what this adds is that the oracle is not fitted to the goldens."""
import numpy as np
import pytest
import torch

from oracle import geometry as G
from oracle import ref_replay
from oracle.gen_golden import T, _RecordRandperm, _StableSort, tc
from vggsfm_amd.scene import make_scene, perturb_for_ba

REF = ref_replay.calls("oracle_live_vs_reference")
helpers = REF.module("vggsfm.utils.triangulation_helpers")
tri = REF.module("vggsfm.utils.triangulation")


def _triangulate_tracks_recording_draws(*args, **kwargs):
    """The reference's triangulate_tracks under a stable sort, with the torch.randperm draws it makes."""
    with _StableSort(), _RecordRandperm() as rec:
        out = ref_replay.reference("vggsfm.utils.triangulation:triangulate_tracks")(*args, **kwargs)
    return out, rec.draws


triangulate_tracks_with_draws = REF.fn("vggsfm.utils.triangulation:triangulate_tracks", _triangulate_tracks_recording_draws)

CASES = [  # seed, S, N, camera, shared
    (101, 7, 90, "SIMPLE_PINHOLE", False),
    (102, 11, 120, "SIMPLE_RADIAL", True),
    (103, 16, 70, "SIMPLE_RADIAL", False),
]


def _scene(seed, S, N, cam, shared):
    sc = make_scene(S, N, cam, shared_camera=shared, seed=seed, outlier_frac=0.08)
    ext, K, extra, pts = perturb_for_ba(sc, seed=seed, rot_deg=0.2, trans=0.01, focal_rel=0.004)
    return sc, ext, K, extra, pts


@pytest.mark.parametrize("seed,S,N,cam,shared", CASES)
def test_projection_normalisation_and_filter_live(seed, S, N, cam, shared):
    sc, ext, K, extra, pts = _scene(seed, S, N, cam, shared)
    pts = pts.copy()
    pts[0] = [0.0, 0.0, -2.0]                                   # behind the cameras
    pts[1] = [400.0, 1.0, 4.0]                                  # beyond hard_max
    p2r, pcr = helpers.project_3D_points(T(pts), T(ext), T(K), T(extra), return_points_cam=True)
    p2, pc = G.project_3D_points(pts, ext, K, extra, return_points_cam=True)
    np.testing.assert_allclose(pc, pcr.numpy(), rtol=1e-13, atol=1e-13)
    fin = np.isfinite(p2r.numpy()) & (np.abs(p2r.numpy()) < 1e300)
    np.testing.assert_allclose(p2[fin], p2r.numpy()[fin], rtol=1e-11, atol=1e-9)
    tnr = helpers.cam_from_img(T(sc.tracks), T(K), T(extra)).numpy()
    tn = G.cam_from_img(sc.tracks.astype(np.float64), K, extra)
    np.testing.assert_allclose(tn, tnr, rtol=1e-9, atol=1e-12)
    for chk in (False, True):
        for thr in (4, 1.5):
            mr, dr = helpers.filter_all_points3D(T(pts), T(sc.tracks), T(ext), T(K), T(extra), max_reproj_error=thr,
                                                 check_triangle=chk, return_detail=True)
            m, d = G.filter_all_points3D(pts, sc.tracks.astype(np.float64), ext, K, extra, max_reproj_error=thr,
                                         check_triangle=chk, return_detail=True)
            assert np.array_equal(m, mr.numpy()) and np.array_equal(d, dr.numpy().astype(bool)), (chk, thr)


@pytest.mark.parametrize("seed,S,N,cam,shared", CASES)
def test_triangulate_by_pair_live(seed, S, N, cam, shared):
    sc, ext, K, extra, _ = _scene(seed, S, N, cam, shared)
    tn = helpers.cam_from_img(T(sc.tracks), T(K), T(extra))
    pr, cher, angr = tri.triangulate_by_pair(T(ext)[None], tn[None])
    p, che, ang = G.triangulate_by_pair(ext, tn.numpy())
    assert np.array_equal(che, cher.numpy())
    ok = np.isfinite(pr.numpy()).all(-1)
    np.testing.assert_allclose(p[ok], pr.numpy()[ok], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(ang[ok], angr.numpy()[ok], rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("seed,S,N,cam,iters", [(111, 9, 80, "SIMPLE_PINHOLE", 256), (112, 26, 60, "SIMPLE_RADIAL", 256),
                                               (113, 25, 50, "SIMPLE_PINHOLE", 128)])
def test_triangulate_tracks_live(seed, S, N, cam, iters):
    sc, ext, K, extra, _ = _scene(seed, S, N, cam, cam == "SIMPLE_RADIAL")
    vis, score = sc.vis.copy(), sc.score.copy()
    score[:, ::11] = 0.45                                        # whole tracks below the score threshold
    vis[1, ::7] = 0.04                                           # entries below the visibility threshold
    tn = helpers.cam_from_img(T(sc.tracks), T(K), T(extra))
    torch.manual_seed(seed)
    (pr, numr, mskr), draws = triangulate_tracks_with_draws(T(ext), tc(tn), max_ransac_iters=iters, track_vis=tc(T(vis)),
                                                            track_score=tc(T(score)))
    comb = G.generate_combinations(S)
    if iters > len(comb):
        assert not draws
        pairs = comb
    else:
        assert len(draws) == 1                                   # one chunk, one draw
        pairs = comb[draws[0][:iters]]
    p, num, msk = G.triangulate_tracks_chunk(ext, tn.numpy(), pairs, lo_num=min(50, len(pairs)), track_vis=vis,
                                             track_score=score)
    assert np.array_equal(num, numr.numpy())
    assert np.array_equal(msk, mskr.numpy())
    ok = numr.numpy() >= 2
    np.testing.assert_allclose(p[ok], pr.numpy()[ok], rtol=1e-7, atol=1e-8)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_reference_rejects_nonfinite_rays(bad):
    """ADVICE r3 (a NaN / inf normalised coordinate in a view the track is NOT visible in): the reference does not get as far
    as its all-view mean -- the view pairs of its RANSAC stage include the invisible views, the DLT matrix of such a pair is
    non-finite and ``torch.linalg.eigh`` raises (triangulation_helpers.py:87).  Finite normalised tracks are therefore a
    PRECONDITION of ``triangulate_tracks``; the drop-in raises the same exception type up front
    (vggsfm_amd/utils/triangulation.py), and the kernel's behaviour on such input is defined anyway (every RANSAC hypothesis of
    the track poisoned: tests/test_gpu_triangulation.py::test_nonfinite_ray_in_invisible_view)."""
    seed, S, N = 117, 12, 90
    sc, ext, K, extra, _ = _scene(seed, S, N, "SIMPLE_PINHOLE", False)
    vis = sc.vis.copy()
    tn = helpers.cam_from_img(T(sc.tracks), T(K), T(extra)).numpy().copy()
    vis[S - 1, 3] = 0.0
    tn[S - 1, 3, 0] = bad
    with pytest.raises(torch.linalg.LinAlgError):
        tri.triangulate_tracks(T(ext), tc(T(tn)), max_ransac_iters=256, track_vis=tc(T(vis)), track_score=tc(T(sc.score)))
