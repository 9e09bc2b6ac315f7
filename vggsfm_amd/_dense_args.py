"""The argument checks the dense stage shares (mvs, patchmatch, fusion, meshing): host index arrays, float64 tensors of a
stated shape, and the five inputs of an entry -- maps, poses, cams, rays and which ray map a view uses -- on the device.
Loads no library, so a stage imports it whichever of the other libraries is built."""
import numpy as np
import torch

from ._lib import require_gpu


def host_i32(values):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(values, dtype=np.int64).reshape(-1).astype(np.int32)))


def f64(t, shape, what):
    t = torch.as_tensor(t)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t.to(torch.float64).contiguous()


def maps(t, what):
    """(S,H,W) float32 maps (grey frames, depth maps), contiguous and on the device"""
    t = torch.as_tensor(t)
    if t.dim() != 3 or t.dtype != torch.float32:
        raise ValueError(f"{what} must be (S,H,W) float32, got {tuple(t.shape)} {t.dtype}")
    t = t.contiguous()
    require_gpu(t)
    return t


def views(t, poses, cams):
    """poses (S,3,4) and cams (S,4) of the S maps t, float64 on their device"""
    return f64(poses, (t.shape[0], 3, 4), "poses").to(t.device), f64(cams, (t.shape[0], 4), "cams").to(t.device)


def reference_inputs(frames, poses, cams, ref, rays):
    """What an entry that works on one reference view takes (the sweep, PatchMatch): frames, poses, cams and the ray map
    (H,W,2) of view ref (default: mvs.pixel_rays of its camera), checked and on the device."""
    from .mvs import pixel_rays

    frames = maps(frames, "frames")
    S, H, W = frames.shape
    poses, cams = views(frames, poses, cams)
    if rays is None:
        if not 0 <= ref < S:
            raise ValueError(f"ref {ref} outside [0, {S})")
        rays = pixel_rays(cams[ref], H, W, frames.device)
    rays = f64(rays, (H, W, 2), "rays")
    require_gpu(rays)
    return frames, poses, cams, rays


def all_view_inputs(depth, poses, cams, rays, ray_index):
    """What an entry that works across the views takes (the consistency filter, the fusion): depth, poses, cams, the ray
    maps (NR,H,W,2) and the host ray_index (S,) (default: mvs.camera_rays(cams)), checked and on the device."""
    from .mvs import camera_rays

    depth = maps(depth, "depth")
    S, H, W = depth.shape
    poses, cams = views(depth, poses, cams)
    if rays is None:
        rays, ray_index = camera_rays(cams, H, W, depth.device)
    rays = torch.as_tensor(rays)
    if rays.dim() != 4:
        raise ValueError(f"rays must be (NR,H,W,2), got {tuple(rays.shape)}")
    rays = f64(rays, (rays.shape[0], H, W, 2), "rays")
    require_gpu(rays)
    if ray_index is None:
        raise ValueError("rays without ray_index")
    ridx = host_i32(ray_index)
    if ridx.numel() != S:
        raise ValueError(f"ray_index must have {S} entries, got {ridx.numel()}")
    return depth, poses, cams, rays, ridx
