"""A camera prior from tracks alone: what the Triangulator otherwise gets from VGGSfM's learned camera
predictor, built from the geometric blocks of this package.  No counterpart in the reference, which always has its predictor;
the recipe is COLMAP's incremental mapper restricted to what the existing kernels do for all frames at once:

    two-view stage    ``estimate_preliminary_cameras(decompose=True)``: (R_s, t_s) of every pair (0, s), each in ITS OWN unit
                      baseline -- so these cameras alone share no scale
    initial pair      ``triangulate_by_pair`` + ``find_best_initial_pair`` (triangulator.py:442-476): the pair (0, s*) fixes the
                      world (frame 0) and the gauge (its unit baseline); its inlier points are the first point set
    registration      rounds of ``absolute_pose_estimation_batch`` (P3P RANSAC + EPnP local optimisation + refinement) over ALL
                      unregistered frames at once, against the points so far; after a round that registered something,
                      ``triangulate_tracks`` over the registered frames extends the point set

With ``estimate_focal_length`` the focal of the two-view stage is not the default one but the value of COLMAP's focal factor
grid under which the fundamental matrices come closest to essential matrices (``sweep_focal_factor``), and the registrations
sweep the grid again, per frame.

Everything stays on the device; the loop reads back one (S,) bool row per round.  A frame that never registers keeps its
two-view pose and is flagged; nothing raises."""
from typing import NamedTuple

import torch

from .. import _lib
from ..ba_options import AbsolutePoseEstimationOptions, AbsolutePoseRefinementOptions
from ..pose import absolute_pose_estimation_batch, focal_length_factors
from ..utils.triangulation import triangulate_by_pair, triangulate_tracks
from ..utils.triangulation_helpers import cam_from_img
from .estimate_preliminary import (decompose_essential_matrix, essential_from_fundamental, estimate_preliminary_cameras,
                                   get_default_intri, remove_cheirality)

VIS_THRES = 0.05            # the reference's two thresholds on a tracker's output (triangulation.py:725-731)
SCORE_THRES = 0.5
INIT_TRI_ANGLE_THRES = 16   # triangulator.py:52


class CameraPrior(NamedTuple):
    """Reads like the camera predictor's output: ``get_EFP(prior, image_size, 1, S)`` gives back `extrinsics` and the focal
    length of `intrinsics`.  R (S,3,3), T (S,3): OpenCV world-to-camera; focal_length (S,2) in NDC units of the short side."""
    R: torch.Tensor
    T: torch.Tensor
    focal_length: torch.Tensor
    registered: torch.Tensor        # (S,) bool: posed by the initial pair or by a registration round
    extrinsics: torch.Tensor        # (S,3,4) f64
    intrinsics: torch.Tensor        # (S,3,3) f64
    rounds: int                     # registration rounds that ran


def make_camera_prior(extrinsics, focal_px, width, height, registered=None, rounds=0):
    """extrinsics (S,3,4), focal_px (S,) pixels -> CameraPrior.  The focal is first brought inside ``get_EFP``'s clamp
    ([0.2, 5] x short side; strictly inside, by 1e-6 of it: ``get_EFP`` rounds its bounds to the dtype of the image size it is
    given) and `intrinsics` is computed from the stored NDC value the way ``get_EFP`` computes it, so the round trip is exact."""
    ext = extrinsics.to(torch.float64).contiguous()
    S = ext.shape[0]
    short = float(min(width, height))
    f = focal_px.to(torch.float64).reshape(S).clamp(0.2 * short * (1 + 1e-6), 5 * short * (1 - 1e-6))
    ndc = (f / (short / 2))[:, None].expand(S, 2).contiguous()
    f_back = (ndc * (short / 2)).mean(dim=-1)
    K = torch.zeros((S, 3, 3), dtype=torch.float64, device=ext.device)
    K[:, 0, 0] = K[:, 1, 1] = f_back
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = width / 2, height / 2, 1.0
    if registered is None:
        registered = torch.ones(S, dtype=torch.bool, device=ext.device)
    return CameraPrior(ext[:, :, :3].contiguous(), ext[:, :, 3].contiguous(), ndc, registered, ext, K, int(rounds))


def _check_arguments(tracks, tracks_vis, tracks_score):
    if tracks.dim() != 4 or tracks.shape[-1] != 2:
        raise ValueError(f"tracks must be (1,S,N,2), got {tuple(tracks.shape)}")
    B, S, N, _ = tracks.shape
    if B != 1:
        raise ValueError(f"one sequence at a time: tracks must be (1,S,N,2), got a batch of {B}")
    if S < 2:
        raise ValueError(f"need at least 2 frames, got {S}")
    if tuple(tracks_vis.shape) != (1, S, N):
        raise ValueError(f"tracks_vis must be (1,{S},{N}), got {tuple(tracks_vis.shape)}")
    if tracks_score is not None and tuple(tracks_score.shape) != (1, S, N):
        raise ValueError(f"tracks_score must be (1,{S},{N}), got {tuple(tracks_score.shape)}")
    return S, N


def _triangulate_registered(ext, tn, vis, score, registered, seed):
    """``triangulate_tracks`` over the registered frames: the others are invisible to it.  Above 256 view pairs it draws its
    hypothesis pairs from torch's global CPU generator (as the reference does); here that draw is seeded from the caller's
    generator and the global state is put back."""
    state = torch.get_rng_state()
    try:
        torch.default_generator.manual_seed(seed)
        return triangulate_tracks(ext, tn, track_vis=vis * registered[:, None].to(vis.dtype), track_score=score)
    finally:
        torch.set_rng_state(state)


def sweep_focal_factor(fmat, width, height, factors):
    """The factor of the default focal under which the fundamental matrices fmat (P,3,3) of the pairs (0, s) look most like
    essential matrices: E = K^T F K of a calibrated pair has two EQUAL non-zero singular values (Huang / Faugeras), so the
    relative gap (s1 - s2) / s1 measures how wrong K is (the self-calibration criterion of Mendonca / Cipolla, CVPR 1999).
    One focal for both frames of every pair, principal point at the image centre; the median over the pairs is taken, so a
    pair whose F rests on a handful of matches does not decide.  Evaluated on COLMAP's grid of focal length factors, the grid
    the registrations sweep as well: its step is the resolution.  Returns a 0-dim tensor; nothing is read back."""
    dev = fmat.device
    g = torch.as_tensor(factors, dtype=torch.float64, device=dev)
    f = g * max(width, height)
    K = torch.zeros((g.numel(), 3, 3), dtype=torch.float64, device=dev)
    K[:, 0, 0] = K[:, 1, 1] = f
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = width / 2, height / 2, 1.0
    E = K.transpose(1, 2)[:, None] @ fmat.to(torch.float64)[None] @ K[:, None]           # (G,P,3,3)
    sv = torch.linalg.svdvals(E)
    gap = (sv[..., 0] - sv[..., 1]) / sv[..., 0].clamp(min=torch.finfo(torch.float64).tiny)
    return g[torch.argmin(gap.median(dim=1).values)]


def two_view_cameras(fmat, tracks, K):
    """The second half of ``estimate_preliminary_cameras`` under a given K (3,3), one camera for all frames: fmat (S-1,3,3),
    tracks (S,N,2) -> (S,3,4) f64, frame 0 the identity, every other frame at unit baseline from it."""
    S = tracks.shape[0]
    dev = tracks.device
    Kp = K[None].expand(S - 1, -1, -1)
    Rs, Ts = decompose_essential_matrix(essential_from_fundamental(fmat.to(torch.float64), Kp, Kp))
    fl = K[0, 0].expand(S - 1, 4)
    pp = torch.stack([K[0, 2], K[1, 2], K[0, 2], K[1, 2]])[None].expand(S - 1, 4)
    R, t = remove_cheirality(Rs, Ts, tracks[0:1].expand(S - 1, -1, -1), tracks[1:], fl, pp)
    first = torch.eye(3, 4, dtype=torch.float64, device=dev)[None]
    return torch.cat([first, torch.cat([R, t[:, :, None]], dim=-1)], dim=0)


def geometric_camera_prior(tracks, tracks_vis, width, height, tracks_score=None, preliminary_dict=None,
                           camera_type="SIMPLE_PINHOLE", shared_camera=False, estimate_focal_length=False, min_num_inliers=30,
                           generator=None):
    """tracks (1,S,N,2) pixels, tracks_vis (1,S,N) [, tracks_score (1,S,N)] -> CameraPrior.

    preliminary_dict: the dictionary of ``estimate_preliminary_cameras``; its two-view cameras (`R_opencv`, `t_opencv`) are
    reused when present, decomposed from its `fmat` when only that is there (``decompose=False``), estimated otherwise.  estimate_focal_length: the default focal (max(width, height)) is only a
    starting point -- the two-view stage takes its focal from COLMAP's grid of focal length factors (``sweep_focal_factor``, on
    the dictionary's `fmat`; one focal for the sequence), the two-view cameras are decomposed under it, and every registration
    sweeps the same grid around it and refines the winner, per frame.  min_num_inliers: COLMAP's
    ``abs_pose_min_num_inliers``.  generator: a generator of the tracks' device for the P3P samples (None: a private one,
    seeded with 0 -- the call is deterministic either way and leaves the global generators alone once the two-view cameras
    are given)."""
    from ..models.triangulator import find_best_initial_pair

    S, N = _check_arguments(tracks, tracks_vis, tracks_score)
    if camera_type not in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL"):
        raise ValueError(f"Camera type {camera_type} is not supported yet")
    _lib.require_gpu(tracks, tracks_vis, tracks_score)
    dev = tracks.device
    if generator is None:
        generator = torch.Generator(device=dev)
        generator.manual_seed(0)
    estopt = AbsolutePoseEstimationOptions(estimate_focal_length=bool(estimate_focal_length))
    estopt.ransac.lo_max_rounds = 10
    refopt = AbsolutePoseRefinementOptions(refine_focal_length=bool(estimate_focal_length))
    # ---- 1. two-view stage: the caller's two-view cameras, else the caller's fundamental matrices decomposed, else both made here
    have = (lambda *keys: preliminary_dict is not None and all(k in preliminary_dict for k in keys))
    cameras_given = have("R_opencv", "t_opencv", "fmat_inlier_mask") and not estimate_focal_length
    if not cameras_given and not have("fmat", "fmat_inlier_mask"):
        _, preliminary_dict = estimate_preliminary_cameras(tracks, tracks_vis, width, height, tracks_score=tracks_score,
                                                           decompose=not estimate_focal_length)
        cameras_given = not estimate_focal_length
    trk, vis = tracks[0], tracks_vis[0]
    score = tracks_score[0] if tracks_score is not None else None
    f0, _, K0 = get_default_intri(width, height, dev, torch.float64)
    if estimate_focal_length:
        # the default focal may be far off, and cameras decomposed from K^T F K with a wrong K give a distorted point set
        # that no later sweep repairs: pick the focal of the two-view stage from the same grid first
        f0 = f0 * sweep_focal_factor(preliminary_dict["fmat"][0], width, height, focal_length_factors(estopt))
        K0 = K0.clone()
        K0[0, 0] = K0[1, 1] = f0
    if cameras_given:
        ext = torch.cat([preliminary_dict["R_opencv"][0], preliminary_dict["t_opencv"][0][:, :, None]], dim=-1).to(torch.float64)
    else:
        ext = two_view_cameras(preliminary_dict["fmat"][0], trk, K0)
    K = K0[None].repeat(S, 1, 1)
    # ---- 2. initial pair (0, s*): world = frame 0, gauge = its unit baseline
    tn = cam_from_img(trk, K)
    pts_pair, cheirality_pair, angle_pair = triangulate_by_pair(ext[None], tn[None])
    inlier_geo_vis = torch.logical_and(preliminary_dict["fmat_inlier_mask"][0], (vis > VIS_THRES)[1:])
    inlier_total, _ = find_best_initial_pair(inlier_geo_vis, cheirality_pair, angle_pair, INIT_TRI_ANGLE_THRES)
    init_idx = torch.argmax(inlier_total.sum(dim=-1))
    has_point = inlier_total[init_idx]
    points = torch.where(has_point[:, None], pts_pair[init_idx], torch.zeros((), dtype=torch.float64, device=dev))
    registered = torch.zeros(S, dtype=torch.bool, device=dev)
    registered[0] = True
    registered[init_idx + 1] = True
    # ---- 3. registration rounds
    usable = vis > VIS_THRES
    if score is not None:
        usable = usable & (score >= SCORE_THRES)
    params = torch.zeros((S, 4), dtype=torch.float64, device=dev)             # COLMAP rows (f, cx, cy, k)
    params[:, 0], params[:, 1], params[:, 2] = f0, width / 2, height / 2
    flags = torch.full((S,), 1 if estimate_focal_length else 0, dtype=torch.uint8, device=dev)
    on_host = registered.cpu()
    rounds = 0
    while rounds < S - 2 and not bool(on_host.all()):
        ids = torch.nonzero(~on_host).squeeze(1).to(dev)
        new_ext, new_params, success, num_inliers, _ = absolute_pose_estimation_batch(
            ext, params, trk, points, usable & has_point[None], ids, camera_type, flags, estopt, refopt, generator=generator)
        rounds += 1
        accept = success & (num_inliers >= min_num_inliers) & ~registered
        ext = torch.where(accept[:, None, None], new_ext, ext)
        params = torch.where(accept[:, None], new_params, params)
        registered = registered | accept
        before, on_host = on_host, registered.cpu()                            # the round's one readback
        if bool((on_host == before).all()) or bool(on_host.all()):
            break
        if estimate_focal_length:
            K = K.clone()
            K[:, 0, 0] = K[:, 1, 1] = params[:, 0]
            tn = cam_from_img(trk, K)
        pts, num, _ = _triangulate_registered(ext, tn, vis, score, registered, generator.initial_seed() + rounds)
        fresh = (num >= 2) & ~has_point
        points = torch.where(fresh[:, None], pts, points)
        has_point = has_point | fresh
    focal = params[:, 0]
    if shared_camera:
        focal = ((focal * registered).sum() / registered.sum()).expand(S)
    return make_camera_prior(ext, focal, width, height, registered, rounds)
