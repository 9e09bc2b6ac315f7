"""PatchMatch slanted-plane refinement of the multi-view stereo: a depth AND a normal per pixel, as HIP kernels
(csrc/patchmatch/patchmatch.hip); no namesake in the reference.  The sweep of vggsfm_amd.mvs scores
fronto-parallel planes only; here every pixel of the reference view holds a plane (alpha, beta, gamma) of its camera frame
on which the inverse depth is affine in the ray coordinates, w(u, v) = alpha u + beta v + gamma, scored by the sweep's own
ZNCC cost, and improved by red-black propagation from its neighbours and by random perturbation.

    plane_init                  a depth map (and optionally a normal map) -> the plane state
    plane_cost                  the cost of a plane state, for every pixel
    step                        one half-iteration on one colour of the checkerboard, in place
    outputs                     plane state and costs -> depth, conf, normal
    refine_depth                sweep (or a given start) -> 2 x iterations steps -> Refined(depth, conf, normal, plane, cost)
    dense_depth_from_frames     reconstruction + frames -> depth_dict, conf_dict, normal_dict (sweep, refine, filter)

A point (x, y) with integer coordinates is the centre of pixel [y][x]; depth 0 means "no depth", a normal (0, 0, 0) "no
normal".  What is torch here is plumbing: allocation and the loops over the iterations and the views, neither of which
synchronises with the host."""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib_patchmatch as PM
from . import mvs
from ._lib_patchmatch import check, require_gpu, stream_ptr
from ._dense_args import f64, host_i32, reference_inputs

_L = PM.lib()         # no fallback: importing the refinement without its library is an error

Refined = namedtuple("Refined", "depth conf normal plane cost")


def _range(depth_near, depth_far):
    if not (depth_near > 0 and depth_far > 0 and np.isfinite(depth_near) and np.isfinite(depth_far)):
        raise ValueError(f"depth_near and depth_far must be positive and finite, got {depth_near} and {depth_far}")
    return 1.0 / depth_far, 1.0 / depth_near


def tilt_cos(max_tilt_deg):
    """cos_max_tilt of the entries: the cosine of the largest angle between a plane's normal and the pixel's ray"""
    if not 0.0 <= max_tilt_deg <= 90.0:
        raise ValueError(f"max_tilt_deg must lie in [0, 90], got {max_tilt_deg}")
    return min(max(math.cos(math.radians(max_tilt_deg)), 0.0), 1.0)


def _seed(seed):
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must lie in [0, 2^64), got {seed}")
    return seed


def default_depth_step(depth_near, depth_far, num_planes):
    """two plane spacings of a sweep of num_planes planes over the range"""
    w_far, w_near = _range(depth_near, depth_far)
    return 2.0 * (w_near - w_far) / (num_planes - 1) if num_planes > 1 else 2.0 * (w_near - w_far)


def _state(t, shape, what, dev):
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != torch.float64 or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {tuple(shape)} float64 tensor")
    require_gpu(t)
    if t.device != dev:
        raise ValueError(f"{what} is on {t.device}, the frames on {dev}")
    return t


def plane_init(depth, poses, ref, rays, depth_near, depth_far, normals=None, max_tilt_deg=75.0, seed=0):
    """depth (H,W) float32 (0: none) of view `ref`, poses (S,3,4), rays (H,W,2) its ray map, normals (H,W,3) float32
    world-frame or None -> plane (H,W,3) float64: fronto-parallel at the pixel's depth, or through the pixel's point with its
    normal where that plane is legal; a pixel without depth starts fronto-parallel at a hashed inverse depth of the range."""
    depth = torch.as_tensor(depth)
    if depth.dim() != 2 or depth.dtype != torch.float32:
        raise ValueError(f"depth must be (H,W) float32, got {tuple(depth.shape)} {depth.dtype}")
    depth = depth.contiguous()
    require_gpu(depth)
    H, W = depth.shape
    dev = depth.device
    poses = torch.as_tensor(poses)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise ValueError(f"poses must be (S,3,4), got {tuple(poses.shape)}")
    poses = poses.to(torch.float64).contiguous().to(dev)
    rays = f64(rays, (H, W, 2), "rays")
    require_gpu(rays)
    if normals is not None:
        if tuple(normals.shape) != (H, W, 3) or normals.dtype != torch.float32:
            raise ValueError(f"normals must be {(H, W, 3)} float32, got {tuple(normals.shape)} {normals.dtype}")
        normals = normals.contiguous()
        require_gpu(normals)
    w_far, w_near = _range(depth_near, depth_far)
    plane = torch.empty(H, W, 3, dtype=torch.float64, device=dev)
    check(_L.vggr_plane_init(depth, normals, poses, rays, poses.shape[0], H, W, ref, w_far, w_near, tilt_cos(max_tilt_deg),
                             _seed(seed), plane, stream_ptr()), "vggr_plane_init")
    return plane


def plane_cost(frames, poses, cams, ref, sources, plane, radius=2, min_views=1, min_variance=1e-4, rays=None):
    """frames (S,H,W) float32 grey, poses (S,3,4), cams (S,4), plane (H,W,3) float64 -> cost (H,W) float64: per pixel of view
    `ref` the sweep's cost (mean of 1 - ZNCC over the valid sources, +inf with fewer than min_views or too little variance)
    of that pixel's plane.  The plane (0, 0, w_j) gives the bits of mvs.plane_sweep(..., return_cost=True).cost[j]."""
    frames, poses, cams, rays = reference_inputs(frames, poses, cams, ref, rays)
    S, H, W = frames.shape
    plane = _state(plane, (H, W, 3), "plane", frames.device)
    src = host_i32(sources)
    cost = torch.empty(H, W, dtype=torch.float64, device=frames.device)
    check(_L.vggr_plane_cost(frames, poses, cams, rays, S, H, W, ref, src, src.numel(), radius, min_views, min_variance, plane,
                             cost, stream_ptr()), "vggr_plane_cost")
    return cost


def step(frames, poses, cams, ref, sources, plane, cost, depth_near, depth_far, iteration, colour, depth_step, slope_step=0.5,
         max_tilt_deg=75.0, radius=2, min_views=1, min_variance=1e-4, seed=0, rays=None):
    """One half-iteration on the pixels with (x + y) & 1 == colour: plane (H,W,3) and cost (H,W) float64 are updated in
    place (and returned).  Asynchronous."""
    frames, poses, cams, rays = reference_inputs(frames, poses, cams, ref, rays)
    S, H, W = frames.shape
    plane = _state(plane, (H, W, 3), "plane", frames.device)
    cost = _state(cost, (H, W), "cost", frames.device)
    w_far, w_near = _range(depth_near, depth_far)
    src = host_i32(sources)
    check(_L.vggr_step(frames, poses, cams, rays, S, H, W, ref, src, src.numel(), radius, min_views, min_variance, w_far, w_near,
                       depth_step, slope_step, tilt_cos(max_tilt_deg), _seed(seed), iteration, colour, plane, cost, stream_ptr()),
          "vggr_step")
    return plane, cost


def outputs(plane, cost, poses, ref, rays, min_conf=0.5):
    """plane (H,W,3), cost (H,W) float64 -> depth (H,W), conf (H,W), normal (H,W,3) float32: depth = 1 / w at the pixel's own
    ray, conf = 1 - cost, the unit world normal facing the camera; depth 0 and normal (0, 0, 0) where the cost is not
    finite or conf < min_conf."""
    if not torch.is_tensor(plane) or plane.dim() != 3:
        raise ValueError("plane must be a (H,W,3) float64 tensor")
    H, W = plane.shape[:2]
    require_gpu(plane)
    dev = plane.device
    plane, cost = _state(plane, (H, W, 3), "plane", dev), _state(cost, (H, W), "cost", dev)
    poses = torch.as_tensor(poses)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise ValueError(f"poses must be (S,3,4), got {tuple(poses.shape)}")
    poses = poses.to(torch.float64).contiguous().to(dev)
    rays = f64(rays, (H, W, 2), "rays")
    require_gpu(rays)
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    conf = torch.empty(H, W, dtype=torch.float32, device=dev)
    normal = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    check(_L.vggr_outputs(plane, cost, poses, rays, poses.shape[0], H, W, ref, min_conf, depth, conf, normal, stream_ptr()),
          "vggr_outputs")
    return depth, conf, normal


def refine_depth(frames, poses, cams, ref, sources, depth_near, depth_far, init_depth=None, init_normals=None, iterations=4,
                 radius=2, min_views=1, min_variance=1e-4, min_conf=0.5, seed=0, depth_step=None, slope_step=0.5,
                 max_tilt_deg=75.0, rays=None, num_planes=128):
    """frames (S,H,W) float32 grey, poses (S,3,4), cams (S,4) -> Refined(depth (H,W), conf (H,W), normal (H,W,3) float32,
    plane (H,W,3), cost (H,W) float64) of view `ref` against `sources` (1 .. 8 other views).

    The start is init_depth (H,W) float32 (0: none), with init_normals (H,W,3) float32 world normals where they give a legal
    plane; without init_depth, mvs.plane_sweep with `num_planes` planes.  Then `iterations` iterations of two half-steps
    (colour 0, colour 1), perturbations scaled by 2^-iteration, with no host synchronisation in the loop.  depth_step: the
    scale of the inverse-depth perturbation (default: two plane spacings of a sweep of num_planes planes); slope_step: that
    of the slopes, relative to the pixel's inverse depth; max_tilt_deg: the largest angle between a plane's normal and the
    pixel's ray.  iterations = 0 returns the start.  What the entries refuse (vggsfm_amd_patchmatch.h) raises RuntimeError."""
    frames, poses, cams, rays = reference_inputs(frames, poses, cams, ref, rays)
    if iterations < 0:
        raise ValueError(f"iterations must be >= 0, got {iterations}")
    if init_depth is None:
        init_depth = mvs.plane_sweep(frames, poses, cams, ref, sources, depth_near, depth_far, num_planes, radius, min_views,
                                     min_variance, min_conf, rays=rays).depth
    if depth_step is None:
        depth_step = default_depth_step(depth_near, depth_far, num_planes)
    plane = plane_init(init_depth, poses, ref, rays, depth_near, depth_far, init_normals, max_tilt_deg, seed)
    cost = plane_cost(frames, poses, cams, ref, sources, plane, radius, min_views, min_variance, rays)
    for it in range(int(iterations)):
        for colour in (0, 1):
            step(frames, poses, cams, ref, sources, plane, cost, depth_near, depth_far, it, colour, depth_step, slope_step,
                 max_tilt_deg, radius, min_views, min_variance, seed, rays)
    depth, conf, normal = outputs(plane, cost, poses, ref, rays, min_conf)
    return Refined(depth, conf, normal, plane, cost)


def dense_depth_from_frames(reconstruction, images, iterations=4, seed=0, num_sources=4, min_angle_deg=2.0, num_planes=128,
                            radius=2, min_views=1, min_variance=1e-4, min_conf=0.5, rel_depth_tol=0.01, reproj_tol=1.0,
                            min_consistent=2, range_percentiles=mvs.RANGE_PERCENTILES, range_widen=mvs.RANGE_WIDEN,
                            depth_step=None, slope_step=0.5, max_tilt_deg=75.0):
    """mvs.dense_depth_from_frames with the refinement between the sweep and the consistency check: every registered image
    swept against its source views, refined by `iterations` PatchMatch iterations, and the REFINED maps checked against
    each other.  The bookkeeping (source views, ranges, ray maps, the caps of min_views and min_consistent) is the
    stereo's.  Returns (depth_dict, conf_dict, normal_dict) keyed by image name: (H,W), (H,W) and (H,W,3) float32 device
    tensors; depth 0 and normal (0, 0, 0) where there is none."""
    from . import dense_depth as DD

    grey = mvs.grey_frames(images)
    require_gpu(grey)
    dev = grey.device
    ids = sorted(int(i) for i in reconstruction.reg_image_ids())
    H, W = grey.shape[-2:]
    for i in ids:
        c = reconstruction.cameras[reconstruction.images[i].camera_id]
        if (int(c.height), int(c.width)) != (H, W):
            raise ValueError(f"frames are {H} x {W} but the camera of image {i} is {int(c.height)} x {int(c.width)}")
        if not 0 <= i < grey.shape[0]:
            raise ValueError(f"image id {i} has no frame: {grey.shape[0]} frames")
    pose, cam = DD._camera_rows(reconstruction, ids)
    depth_dict, conf_dict, normal_dict = {}, {}, {}
    if not ids:
        return depth_dict, conf_dict, normal_dict
    row = {i: r for r, i in enumerate(ids)}
    names = [reconstruction.images[i].name for i in ids]
    frames = grey[torch.as_tensor(ids, device=dev)].contiguous()
    poses, cams = torch.from_numpy(pose).to(dev), torch.from_numpy(cam).to(dev)
    rays, ray_index = mvs.camera_rays(cam, H, W, dev)
    sources = mvs.select_source_views(reconstruction, num_sources, min_angle_deg)
    ranges = mvs.depth_ranges(reconstruction, range_percentiles, range_widen, dev)
    raw = torch.zeros(len(ids), H, W, dtype=torch.float32, device=dev)
    normals = torch.zeros(len(ids), H, W, 3, dtype=torch.float32, device=dev)
    for r, i in enumerate(ids):
        src = [row[j] for j in sources[i]]
        conf_dict[names[r]] = torch.zeros(H, W, dtype=torch.float32, device=dev)
        if src and names[r] in ranges:
            near, far = ranges[names[r]]
            out = refine_depth(frames, poses, cams, r, src, near, far, None, None, iterations, radius, min(min_views, len(src)),
                               min_variance, min_conf, seed, depth_step, slope_step, max_tilt_deg, rays[int(ray_index[r])],
                               num_planes)
            raw[r], normals[r], conf_dict[names[r]] = out.depth, out.normal, out.conf
    for r, i in enumerate(ids):
        src = [row[j] for j in sources[i]]
        if src:
            depth_dict[names[r]] = mvs.filter_consistent(raw, poses, cams, r, src, rel_depth_tol, reproj_tol,
                                                         min(min_consistent, len(src)), rays, ray_index).depth
        else:
            depth_dict[names[r]] = raw[r].clone()
        normal_dict[names[r]] = normals[r] * (depth_dict[names[r]] > 0)[..., None]
    return depth_dict, conf_dict, normal_dict
