"""Sim(3) alignment of 3D-3D correspondences on the device (csrc/sim3.hip, prefix ``vggs_``): the weighted Umeyama fit, a
3-point LO-RANSAC around it, and what to do with the result.  Convention: ``tgt ~ scale * R @ src + t``.  Tensors in,
tensors out, float64, on the caller's stream; nothing here synchronises with the host.  DESIGN.md section 20."""
import numpy as np
import torch

from . import _lib


def _batched(src, tgt):
    if src.shape != tgt.shape or src.dim() not in (2, 3) or src.shape[-1] != 3:
        raise ValueError(f"src and tgt must both be (N,3) or (B,N,3), got {tuple(src.shape)} and {tuple(tgt.shape)}")
    single = src.dim() == 2
    s = src.to(torch.float64).reshape((-1,) + tuple(src.shape[-2:])).contiguous()
    t = tgt.to(torch.float64).reshape(s.shape).contiguous()
    return s, t, single


def _per_point(x, B, N, name, dtype):
    if x is None:
        return None
    if tuple(x.shape) not in ((B, N), (N,)) or (x.dim() == 1 and B != 1):
        raise ValueError(f"{name} must be (B,N) = ({B},{N}), got {tuple(x.shape)}")
    return x.to(dtype).reshape(B, N).contiguous()


def _workspace(L, B, N, H, device):
    nbytes = int(L.vggs_sim3_workspace_bytes(B, N, H))
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device), nbytes


def _split(T, single):
    scale, R, t = T[:, 0], T[:, 1:10].reshape(-1, 3, 3), T[:, 10:13]
    return (scale[0], R[0], t[0]) if single else (scale, R, t)


def estimate_sim3(src, tgt, weights=None, estimate_scale=True):
    """Weighted Umeyama.  src, tgt (N,3) or (B,N,3); weights (B,N) >= 0 (a bool mask is the 0/1 case) or None.  Returns
    (scale, R, t, valid): () / (3,3) / (3,) / () for one problem, with a leading B otherwise.  valid is False, and the
    transform the identity, when fewer than 3 points carry weight, the source has no extent or is collinear."""
    s, t, single = _batched(src, tgt)
    B, N, _ = s.shape
    w = _per_point(weights, B, N, "weights", torch.float64)
    _lib.require_gpu(s, t, w)
    L = _lib.lib()
    T = torch.empty((B, 13), dtype=torch.float64, device=s.device)
    valid = torch.empty((B,), dtype=torch.uint8, device=s.device)
    if N == 0:
        T.copy_(torch.tensor([1.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float64))
        valid.zero_()
    else:
        ws, nbytes = _workspace(L, B, N, 0, s.device)
        _lib.check(L.vggs_sim3_fit(s, t, w, B, N, 1 if estimate_scale else 0, T, valid, ws, nbytes, _lib.stream_ptr()),
                   "vggs_sim3_fit")
    scale, R, tr = _split(T, single)
    return scale, R, tr, (valid[0] if single else valid).bool()


def score_sim3(src, tgt, scale, R, t, valid, max_error, mask=None):
    """Support of H given transforms per problem: scale (B,H), R (B,H,3,3), t (B,H,3), valid (B,H); max_error a scalar or
    (B,).  Returns (counts (B,H) int32, -1 where invalid; sums (B,H) of the inliers' squared residuals)."""
    s, tg, _ = _batched(src, tgt)
    B, N, _ = s.shape
    H = valid.reshape(B, -1).shape[1]
    T = torch.cat([scale.reshape(B, H, 1), R.reshape(B, H, 9), t.reshape(B, H, 3)], dim=-1).to(torch.float64).contiguous()
    v = valid.reshape(B, H).to(torch.uint8).contiguous()
    m = _per_point(mask, B, N, "mask", torch.uint8)
    _lib.require_gpu(s, tg, T, v, m)
    thr = _thresholds(max_error, B, s.device)
    L = _lib.lib()
    counts = torch.empty((B, H), dtype=torch.int32, device=s.device)
    sums = torch.empty((B, H), dtype=torch.float64, device=s.device)
    if N == 0:
        counts.copy_(v.to(torch.int32) - 1)
        sums.zero_()
        return counts, sums
    ws, nbytes = _workspace(L, B, N, H, s.device)
    _lib.check(L.vggs_sim3_score(s, tg, m, T, v, thr, B, N, H, counts, sums, ws, nbytes, _lib.stream_ptr()), "vggs_sim3_score")
    return counts, sums


def _thresholds(max_error, B, device):
    if isinstance(max_error, torch.Tensor):
        thr = max_error.to(device=device, dtype=torch.float64).reshape(-1)
        thr = thr.expand(B) if thr.numel() == 1 else thr
    else:
        thr = torch.full((B,), float(max_error), dtype=torch.float64, device=device)
    if thr.shape != (B,):
        raise ValueError(f"max_error must be a scalar or one value per problem ({B}), got {tuple(thr.shape)}")
    return thr.contiguous()


def draw_samples(B, N, num_hypotheses, generator=None):
    """(B,H,3) int32 point indices, drawn on the host (a numpy or CPU torch Generator, or numpy's global state when None)."""
    if isinstance(generator, torch.Generator):
        return torch.randint(0, max(N, 1), (B, num_hypotheses, 3), generator=generator, dtype=torch.int32)
    rng = generator if generator is not None else np.random
    draw = rng.integers if hasattr(rng, "integers") else rng.randint
    return torch.from_numpy(np.asarray(draw(0, max(N, 1), size=(B, num_hypotheses, 3))).astype(np.int32))


def estimate_sim3_robust(src, tgt, max_error, mask=None, num_hypotheses=1024, lo_rounds=10, min_inliers=3, estimate_scale=True,
                         samples=None, generator=None, return_scores=False, workspace=None):
    """3-point LO-RANSAC.  src, tgt (N,3) or (B,N,3); max_error a scalar or (B,), in target units; mask (B,N) or None;
    samples (B,H,3) (or (H,3), shared) replays a draw.  Returns (scale, R, t, num_inliers, inliers, success) and, with
    return_scores, also ((counts, sums) of the minimal hypotheses (B,H), the winning index, the accepted LO rounds).
    The winner: most inliers, then the smaller inlier residual sum, then the lower index."""
    s, t, single = _batched(src, tgt)
    B, N, _ = s.shape
    if int(min_inliers) < 3:
        raise ValueError(f"min_inliers must be >= 3, got {min_inliers}")
    if int(lo_rounds) < 0:
        raise ValueError(f"lo_rounds must be >= 0, got {lo_rounds}")
    if N < 3:
        raise ValueError(f"need at least 3 correspondences, got {N}")
    m = _per_point(mask, B, N, "mask", torch.uint8)
    _lib.require_gpu(s, t, m)
    dev = s.device
    if samples is None:
        if int(num_hypotheses) < 1:
            raise ValueError(f"num_hypotheses must be >= 1, got {num_hypotheses}")
        samples = draw_samples(B, N, int(num_hypotheses), generator)
    smp = torch.as_tensor(samples).to(device=dev, dtype=torch.int32)
    if smp.dim() == 2:
        smp = smp[None].expand(B, -1, -1)
    if smp.dim() != 3 or smp.shape[0] != B or smp.shape[2] != 3 or smp.shape[1] < 1:
        raise ValueError(f"samples must be (B,H,3) or (H,3) with H >= 1, got {tuple(smp.shape)}")
    smp = smp.contiguous()
    H = smp.shape[1]
    thr = _thresholds(max_error, B, dev)
    L = _lib.lib()
    T = torch.empty((B, 13), dtype=torch.float64, device=dev)
    num = torch.empty((B,), dtype=torch.int32, device=dev)
    inl = torch.empty((B, N), dtype=torch.uint8, device=dev)
    rsum = torch.empty((B,), dtype=torch.float64, device=dev)
    best = torch.empty((B,), dtype=torch.int32, device=dev)
    rounds = torch.empty((B,), dtype=torch.int32, device=dev)
    success = torch.empty((B,), dtype=torch.uint8, device=dev)
    counts = torch.empty((B, H), dtype=torch.int32, device=dev) if return_scores else None
    sums = torch.empty((B, H), dtype=torch.float64, device=dev) if return_scores else None
    nbytes = int(L.vggs_sim3_workspace_bytes(B, N, H))
    ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if ws.numel() * ws.element_size() < nbytes:
        raise ValueError(f"workspace holds {ws.numel() * ws.element_size()} bytes, {nbytes} are needed")
    _lib.check(L.vggs_sim3_ransac(s, t, m, thr, smp, B, N, H, int(lo_rounds), int(min_inliers), 1 if estimate_scale else 0,
                                  T, num, inl, rsum, best, rounds, success, counts, sums, ws, nbytes, _lib.stream_ptr()),
               "vggs_sim3_ransac")
    scale, R, tr = _split(T, single)
    pick = (lambda x: x[0]) if single else (lambda x: x)
    out = (scale, R, tr, pick(num), pick(inl.bool()), pick(success.bool()))
    if return_scores:
        out = out + ((pick(counts), pick(sums)), pick(best), pick(rounds))
    return out


def transform_points(points, scale, R, t):
    """scale * R @ p + t for points (...,3)."""
    return scale * (points @ R.transpose(-1, -2)) + t


def transform_extrinsics(extrinsics, scale, R, t):
    """The world-to-camera [R_i|t_i] (S,3,4) that see the world moved by (scale, R, t) as they saw it before, up to the
    scale of the camera frame: R_i' = R_i R^T, t_i' = scale t_i - R_i R^T t (the reference's apply_transformation with
    align_R = R^T, align_T = -R^T t, align_s = scale)."""
    rot = extrinsics[..., :3] @ R.transpose(-1, -2)
    tr = scale * extrinsics[..., 3] - (rot @ t.reshape(3, 1))[..., 0]
    return torch.cat([rot, tr[..., None]], dim=-1)


def camera_centers(extrinsics):
    """Projection centres -R_i^T t_i of (S,3,4) world-to-camera poses."""
    return -(extrinsics[..., :3].transpose(-1, -2) @ extrinsics[..., 3:])[..., 0]


def align_cameras(extrinsics_src, extrinsics_tgt, max_error=None, **ransac):
    """Sim(3) that carries the projection centres of the source cameras (S,3,4) onto the target's: the plain fit when
    max_error is None, the robust one (keywords of `estimate_sim3_robust`) otherwise.  Returns ((scale, R, t, ok), the
    source extrinsics in the target's world)."""
    if extrinsics_src.shape != extrinsics_tgt.shape or extrinsics_src.dim() != 3 or tuple(extrinsics_src.shape[1:]) != (3, 4):
        raise ValueError("extrinsics_src and extrinsics_tgt must both be (S,3,4)")
    src, tgt = extrinsics_src.to(torch.float64), extrinsics_tgt.to(torch.float64)
    cs, ct = camera_centers(src), camera_centers(tgt)
    if max_error is None:
        scale, R, t, ok = estimate_sim3(cs, ct, estimate_scale=ransac.pop("estimate_scale", True))
        if ransac:
            raise TypeError(f"unexpected keywords without max_error: {sorted(ransac)}")
    else:
        scale, R, t, _, _, ok = estimate_sim3_robust(cs, ct, max_error, **ransac)[:6]
    return (scale, R, t, ok), transform_extrinsics(src, scale, R, t)
