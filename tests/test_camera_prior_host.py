"""``vggsfm_amd.two_view_geo.camera_prior`` without a GPU: the argument checks, the ``get_EFP`` round trip of a
``CameraPrior``, and the registration loop driven by a fake backend in the style of tests/cpu_backend.py
-- the DRIVER (who is tried when, what a round's re-triangulation sees, who keeps which pose) is the product's; the two
estimators are scripted, the two-view geometry is oracle/geometry.py."""
import random

import numpy as np
import pytest
import torch

from oracle import geometry as OG
from vggsfm_amd.models.utils import get_EFP
from vggsfm_amd.scene import make_cameras, project
from vggsfm_amd.two_view_geo import CameraPrior, geometric_camera_prior
from vggsfm_amd.two_view_geo import camera_prior as CP

W = H = 1024


def test_argument_checks():
    tr, vis = torch.zeros(1, 4, 10, 2), torch.ones(1, 4, 10)
    bad = [(torch.zeros(4, 10, 2), vis, None), (torch.zeros(1, 4, 10, 3), vis, None), (tr, torch.ones(1, 4, 9), None),
           (tr, torch.ones(4, 10), None), (tr, vis, torch.ones(1, 4, 11)),
           (torch.zeros(1, 1, 10, 2), torch.ones(1, 1, 10), None),                       # S < 2
           (torch.zeros(2, 4, 10, 2), torch.ones(2, 4, 10), None)]                       # B != 1
    for t, v, s in bad:
        with pytest.raises(ValueError):
            geometric_camera_prior(t, v, W, H, tracks_score=s)
    with pytest.raises(ValueError):
        geometric_camera_prior(tr, vis, W, H, camera_type="OPENCV")


@pytest.mark.parametrize("size", [(1024, 1024), (1024, 768), (600, 1000)])
def test_get_EFP_round_trip(size):
    w, h = size
    g = torch.Generator().manual_seed(1)
    S = 7
    ext = torch.randn(S, 3, 4, dtype=torch.float64, generator=g)
    focal = torch.rand(S, dtype=torch.float64, generator=g) * 1500 + 300
    focal[0], focal[1] = 10.0, 1e5                                                      # both outside get_EFP's clamp
    prior = CP.make_camera_prior(ext, focal, w, h, rounds=2)
    assert isinstance(prior, CameraPrior) and prior.rounds == 2 and bool(prior.registered.all())
    short = min(w, h)
    assert abs(float(prior.intrinsics[0, 0, 0]) / (0.2 * short) - 1) < 2e-6 and abs(float(prior.intrinsics[1, 0, 0]) / (5 * short) - 1) < 2e-6
    assert torch.equal(prior.intrinsics[2:, 0, 0], (focal[2:] / (short / 2)) * (short / 2))
    for dtype in (torch.float32, torch.float64):
        e, K = get_EFP(prior, torch.tensor([w, h], dtype=dtype), 1, S)
        assert torch.equal(e[0], ext) and torch.equal(e[0], prior.extrinsics)
        assert torch.equal(K[0], prior.intrinsics) and K.dtype == torch.float64
    # a hand-built one
    hand = CameraPrior(ext[:, :, :3], ext[:, :, 3], torch.full((S, 2), 1.75, dtype=torch.float64), torch.ones(S, dtype=torch.bool),
                       ext, None, 0)
    e, K = get_EFP(hand, torch.tensor([w, h], dtype=torch.float32), 1, S)
    assert torch.equal(e[0], ext) and torch.equal(K[0, :, 0, 0], torch.full((S,), 1.75 * short / 2, dtype=torch.float64))


def test_sweep_focal_factor_on_exact_fundamental_matrices():
    """F = K^-T [t]x R K^-1 of the arc of ``make_cameras`` under one true focal: the sweep lands on a grid value next to it
    (plain torch, runs anywhere), for a truth below, at and above the default focal; a junk pair does not move it."""
    from vggsfm_amd.ba_options import AbsolutePoseEstimationOptions
    from vggsfm_amd.pose import focal_length_factors
    grid = np.array(focal_length_factors(AbsolutePoseEstimationOptions(estimate_focal_length=True)))
    ext, _, _ = make_cameras(8, "SIMPLE_PINHOLE", True, seed=0)
    for w, h, true in ((1024, 1024, 0.7), (1024, 768, 1.0), (640, 480, 1.9)):
        f = true * max(w, h)
        Kinv = np.linalg.inv(np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1.0]]))
        F = []
        for s in range(1, 8):
            R, t = ext[s, :, :3], ext[s, :, 3]
            tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
            F.append(Kinv.T @ tx @ R @ Kinv)
        F[2] = np.random.default_rng(0).normal(size=(3, 3))
        got = float(CP.sweep_focal_factor(torch.from_numpy(np.stack(F)), w, h, grid.tolist()))
        hi = int(np.searchsorted(grid, true))
        assert got in (grid[hi - 1], grid[hi]), (true, got)


# ---------------------------------------------------------------------------------------------------------------------
S, N, N_INIT = 6, 200, 120


def _two_view_world():
    """Noise-free tracks of 6 cameras on the arc of ``make_cameras``, every track visible everywhere, and the exact two-view
    cameras (R_s, t_s / |t_s|); only the first N_INIT tracks are fundamental-matrix inliers, so the initial pair's point set
    leaves something for a re-triangulation to add."""
    ext, K, _ = make_cameras(S, "SIMPLE_PINHOLE", True, seed=0, focal=float(W))          # focal = the default intrinsics
    rng = np.random.default_rng(0)
    pts = np.array([0.0, 0.0, 4.0]) + rng.uniform(-1, 1, (N, 3))
    uv, _ = project(pts, ext, K, None)
    t = ext[:, :, 3].copy()
    t[1:] /= np.linalg.norm(t[1:], axis=1, keepdims=True)
    mask = np.zeros((1, S - 1, N), bool)
    mask[..., :N_INIT] = True
    prelim = {"R_opencv": torch.from_numpy(ext[:, :, :3].copy())[None], "t_opencv": torch.from_numpy(t)[None],
              "fmat_inlier_mask": torch.from_numpy(mask)}
    return torch.from_numpy(uv.astype(np.float32))[None], torch.ones(1, S, N), prelim


class FakeBackend:
    """Of the frames the first round is asked for, in order: A registers at once, B only once the point set has grown past
    the initial pair's, C always "succeeds" one inlier short of the minimum."""

    def __init__(self, monkeypatch):
        import vggsfm_amd._lib as LIB
        monkeypatch.setattr(LIB, "require_gpu", lambda *t: None)
        monkeypatch.setattr(CP, "cam_from_img", lambda tr, K, ep=None: torch.from_numpy(
            OG.cam_from_img(tr.double().numpy(), K.numpy(), None)))
        monkeypatch.setattr(CP, "triangulate_by_pair", lambda e, tn: tuple(
            torch.from_numpy(a) for a in OG.triangulate_by_pair(e[0].numpy(), tn[0].numpy())))
        monkeypatch.setattr(CP, "absolute_pose_estimation_batch", self.absolute_pose_estimation_batch)
        monkeypatch.setattr(CP, "triangulate_tracks", self.triangulate_tracks)
        self.abc, self.pnp_calls, self.tri_calls = None, [], []

    def absolute_pose_estimation_batch(self, extrinsics, intr_params, points2D, points3D, candidate_mask, frame_ids,
                                       camera_type, refine_flags, estoptions=None, refopts=None, generator=None):
        ids = [int(i) for i in frame_ids]
        if self.abc is None:
            self.abc = ids[:3]
        a, b, c = self.abc
        self.pnp_calls.append(dict(ids=ids, candidates=candidate_mask.sum(1).tolist(), points=points3D.clone(),
                                   lo=estoptions.ransac.lo_max_rounds, focal_sweep=estoptions.estimate_focal_length,
                                   generator=generator))
        ext, intr = extrinsics.clone(), intr_params.clone()
        success = torch.zeros(S, dtype=torch.bool)
        num = torch.zeros(S, dtype=torch.int32)
        for f in ids:
            grown = int(candidate_mask[f].sum()) > N_INIT
            if f == a or (f == b and grown):
                success[f], num[f] = True, 30
            elif f == c:
                success[f], num[f] = True, 29
            if success[f]:
                ext[f] = torch.eye(3, 4, dtype=torch.float64) * (100 + f)                # a pose nobody else produces
        return ext, intr, success, num, candidate_mask.clone()

    def triangulate_tracks(self, extrinsics, tracks_normalized, track_vis=None, track_score=None, **kw):
        torch.randperm(300)                                                              # the device entry draws like this above 256 pairs
        self.tri_calls.append(dict(seen=(track_vis.sum(1) > 0).tolist(), ext=extrinsics.clone()))
        n = tracks_normalized.shape[1]
        return torch.full((n, 3), 7.0, dtype=torch.float64), torch.full((n,), 2, dtype=torch.int64), None


def test_round_loop_on_a_fake_backend(monkeypatch):
    fake = FakeBackend(monkeypatch)
    tracks, vis, prelim = _two_view_world()
    gen = torch.Generator().manual_seed(5)
    prior = geometric_camera_prior(tracks, vis, W, H, preliminary_dict=prelim, generator=gen)
    two_view = torch.cat([prelim["R_opencv"][0], prelim["t_opencv"][0][:, :, None]], -1)
    a, b, c = fake.abc
    init = sorted(set(range(S)) - {a, b, c})
    assert len(init) == 3 and init[0] == 0                                               # frame 0, s*, and the frame beyond C
    reg = prior.registered.tolist()
    assert reg[a] and reg[b] and not reg[c] and reg[0] and reg[init[1]]
    assert prior.rounds == 3 <= S - 2 and len(fake.pnp_calls) == 3
    # who was asked when: all unregistered frames at once, every round
    assert fake.pnp_calls[0]["ids"][:3] == [a, b, c] and a not in fake.pnp_calls[1]["ids"] and b in fake.pnp_calls[1]["ids"]
    assert b not in fake.pnp_calls[2]["ids"] and c in fake.pnp_calls[2]["ids"]
    assert all(k["lo"] == 10 and k["focal_sweep"] is False and k["generator"] is gen for k in fake.pnp_calls)
    # candidates = the tracks that have a point: the initial pair's inliers first, everything after the re-triangulation;
    # the first points stay as they were (the set is extended)
    assert fake.pnp_calls[0]["candidates"][b] == N_INIT and fake.pnp_calls[1]["candidates"][b] == N
    p0, p1 = fake.pnp_calls[0]["points"], fake.pnp_calls[1]["points"]
    assert torch.equal(p0[:N_INIT], p1[:N_INIT]) and bool((p0[N_INIT:] == 0).all()) and bool((p1[N_INIT:] == 7.0).all())
    gt = p0[:N_INIT] / p0[:N_INIT].norm(dim=1, keepdim=True)                             # frame 0 is the world: same rays
    ray = torch.cat([OG_rays(tracks[0, 0, :N_INIT]), torch.ones(N_INIT, 1, dtype=torch.float64)], 1)
    assert float((gt - ray / ray.norm(dim=1, keepdim=True)).abs().max()) < 1e-5
    # a re-triangulation after each round that registered something, over the registered frames only
    assert len(fake.tri_calls) == 2
    assert fake.tri_calls[0]["seen"] == [f in (0, init[1], a) for f in range(S)]
    assert fake.tri_calls[1]["seen"] == [f in (0, init[1], a, b) for f in range(S)]
    assert torch.equal(fake.tri_calls[0]["ext"][a], torch.eye(3, 4, dtype=torch.float64) * (100 + a))
    # poses: A and B what the estimator gave, C and the initial pair their two-view pose
    assert torch.equal(prior.extrinsics[a], torch.eye(3, 4, dtype=torch.float64) * (100 + a))
    assert torch.equal(prior.extrinsics[b], torch.eye(3, 4, dtype=torch.float64) * (100 + b))
    assert torch.equal(prior.extrinsics[c], two_view[c]) and torch.equal(prior.extrinsics[init[1]], two_view[init[1]])
    assert bool((prior.intrinsics[:, 0, 0] == W).all())
    # min_num_inliers is an option: one inlier fewer is enough for C as well
    fake2 = FakeBackend(monkeypatch)
    prior2 = geometric_camera_prior(tracks, vis, W, H, preliminary_dict=prelim, generator=gen, min_num_inliers=29)
    assert fake2.abc == [a, b, c] and bool(prior2.registered[c])


def OG_rays(uv):
    return (uv.double() - W / 2) / W


@pytest.mark.parametrize("with_generator", [True, False])
def test_global_rng_state_untouched(monkeypatch, with_generator):
    FakeBackend(monkeypatch)
    tracks, vis, prelim = _two_view_world()
    torch.manual_seed(11)
    np.random.seed(12)
    random.seed(13)
    before = (torch.get_rng_state().clone(), np.random.get_state(), random.getstate())
    gen = torch.Generator().manual_seed(5) if with_generator else None
    p1 = geometric_camera_prior(tracks, vis, W, H, tracks_score=torch.ones_like(vis), preliminary_dict=prelim, generator=gen)
    assert torch.equal(torch.get_rng_state(), before[0])
    st = np.random.get_state()
    assert st[0] == before[1][0] and np.array_equal(st[1], before[1][1]) and st[2:] == before[1][2:]
    assert random.getstate() == before[2]
    assert p1.rounds == 3
