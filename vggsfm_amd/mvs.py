"""Classical dense depth for users without a depth network: plane-sweep multi-view stereo and the forward-backward
consistency check of the depth maps as HIP kernels (csrc/mvs/mvs.hip); no namesake in the reference,
whose dense stage rescales the maps of a monocular depth model.

    pixel_rays                  the ray map of a camera: cam_from_img (the project's pinned undistortion) on the pixel grid
    plane_sweep                 one reference view against up to 8 sources -> depth, conf, index (and the cost volume)
    filter_consistent           one view's depth map checked against its sources' maps -> depth, count
    select_source_views         host bookkeeping over the track CSR: per image the views that share the most points
    depth_ranges                per image near / far from the percentiles of its sparse depths
    dense_depth_from_frames     reconstruction + frames -> depth_dict, conf_dict (GeometryRunner.dense_reconstruct_from_frames)

A point (x, y) with integer coordinates is the centre of pixel [y][x]; depth 0 and index -1 mean "no depth".  What is torch
here is plumbing: the grey conversion, the pixel grid and the loop over the views."""
from collections import namedtuple

import numpy as np
import torch

from . import _lib_mvs as M
from ._lib_mvs import check, require_gpu, stream_ptr

_L = M.lib()          # no fallback: importing the stereo without its library is an error

# (below the load: without the library, importing this module fails with lib()'s error whatever else is missing)
from ._dense_args import all_view_inputs, host_i32, reference_inputs  # noqa: E402

Sweep = namedtuple("Sweep", "depth conf index cost")
Filtered = namedtuple("Filtered", "depth count")

RANGE_PERCENTILES = (5.0, 95.0)   # depth_ranges: percentiles of the sparse depths ...
RANGE_WIDEN = 1.25                # ... near divided, far multiplied by this factor


def pixel_rays(cam_row, height, width, device=None):
    """(H, W, 2) float64 on the device: the undistorted normalised coordinates of the pixel centres of a camera
    f, cx, cy, k (a row of dense_depth._camera_rows; k = 0: SIMPLE_PINHOLE)."""
    from .utils.triangulation_helpers import cam_from_img

    dev = torch.device("cuda" if device is None else device)
    f, cx, cy, k = (float(v) for v in np.asarray(torch.as_tensor(cam_row).detach().cpu(), np.float64).reshape(4))
    ys, xs = torch.meshgrid(torch.arange(height, dtype=torch.float64, device=dev),
                            torch.arange(width, dtype=torch.float64, device=dev), indexing="ij")
    grid = torch.stack([xs, ys], dim=-1).reshape(1, height * width, 2).contiguous()
    K = torch.tensor([[[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]]], dtype=torch.float64, device=dev)
    extra = torch.tensor([[k]], dtype=torch.float64, device=dev) if k != 0.0 else None
    if height * width == 0:
        return torch.zeros(height, width, 2, dtype=torch.float64, device=dev)
    return cam_from_img(grid, K, extra).reshape(height, width, 2).contiguous()


def camera_rays(cams, height, width, device=None):
    """One ray map per distinct camera row: cams (S,4) -> rays (NR,H,W,2) on the device, ray_index (S,) host int32."""
    rows = np.asarray(torch.as_tensor(cams).detach().cpu(), np.float64).reshape(-1, 4)
    seen, index, maps = {}, [], []
    for row in rows:
        key = row.tobytes()
        if key not in seen:
            seen[key] = len(maps)
            maps.append(pixel_rays(row, height, width, device))
        index.append(seen[key])
    return torch.stack(maps), host_i32(index)


def plane_sweep(frames, poses, cams, ref, sources, depth_near, depth_far, num_planes=128, radius=2, min_views=1,
                min_variance=1e-4, min_conf=0.5, return_cost=False, rays=None):
    """frames (S,H,W) float32 grey, poses (S,3,4), cams (S,4) -> Sweep(depth (H,W) float32, conf (H,W) float32, index (H,W)
    int32, cost (D,H,W) float64 or None) of view `ref` against `sources` (1 .. 8 other views), planes uniform in inverse
    depth between depth_far and depth_near.  rays: the ray map of view ref (default: pixel_rays of its camera).  What the
    entry refuses (vggsfm_amd_mvs.h) raises RuntimeError."""
    frames, poses, cams, rays = reference_inputs(frames, poses, cams, ref, rays)
    S, H, W = frames.shape
    dev = frames.device
    if not (depth_near > 0 and depth_far > 0 and np.isfinite(depth_near) and np.isfinite(depth_far)):
        raise ValueError(f"depth_near and depth_far must be positive and finite, got {depth_near} and {depth_far}")
    src = host_i32(sources)
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    conf = torch.empty(H, W, dtype=torch.float32, device=dev)
    index = torch.empty(H, W, dtype=torch.int32, device=dev)
    cost = torch.empty(int(num_planes), H, W, dtype=torch.float64, device=dev) if return_cost and num_planes > 0 else None
    check(_L.vggm_plane_sweep(frames, poses, cams, rays, S, H, W, ref, src, src.numel(), 1.0 / depth_far, 1.0 / depth_near,
                              num_planes, radius, min_views, min_variance, min_conf, depth, conf, index, cost, stream_ptr()),
          "vggm_plane_sweep")
    return Sweep(depth, conf, index, cost)


def filter_consistent(depth, poses, cams, ref, sources, rel_depth_tol=0.01, reproj_tol=1.0, min_consistent=2, rays=None,
                      ray_index=None):
    """depth (S,H,W) float32 (0: none), poses (S,3,4), cams (S,4) -> Filtered(depth (H,W) float32, count (H,W) int32): the
    depth of view `ref` where at least min_consistent of `sources` confirm it forwards and backwards.  rays (NR,H,W,2) and
    ray_index (S,): the ray maps and which one a view uses (default: camera_rays(cams))."""
    depth, poses, cams, rays, ridx = all_view_inputs(depth, poses, cams, rays, ray_index)
    S, H, W = depth.shape
    dev = depth.device
    src = host_i32(sources)
    out = torch.empty(H, W, dtype=torch.float32, device=dev)
    count = torch.empty(H, W, dtype=torch.int32, device=dev)
    check(_L.vggm_consistency_filter(depth, poses, cams, rays, ridx, rays.shape[0], S, H, W, ref, src, src.numel(),
                                     rel_depth_tol, reproj_tol, min_consistent, out, count, stream_ptr()),
          "vggm_consistency_filter")
    return Filtered(out, count)


# ------------------------------------------------------------------------------------------------ host bookkeeping
def select_source_views(reconstruction, num_sources=4, min_angle_deg=2.0):
    """{image id: [image ids]} over the registered images: per image the (at most) `num_sources` other registered images
    that share the most 3D points whose rays from the two projection centres meet at `min_angle_deg` or more; an image
    that shares no such point is no candidate; equal counts: the lower image id first.  Host code over the track CSR."""
    ids = sorted(int(i) for i in reconstruction.reg_image_ids())
    row = {i: r for r, i in enumerate(ids)}
    ptr, img, _ = reconstruction._track_csr()
    n = len(ptr) - 1
    seen = np.zeros((len(ids), n), bool)
    pid = np.repeat(np.arange(n), np.diff(ptr))
    reg = np.isin(img, ids)
    seen[[row[int(i)] for i in img[reg]], pid[reg]] = True
    xyz = np.asarray(reconstruction._xyz[:n], np.float64)
    centres = np.stack([np.asarray(reconstruction.images[i].projection_center(), np.float64) for i in ids]) if ids else np.zeros((0, 3))
    d = xyz[None] - centres[:, None]                                        # (S, P, 3)
    norm = np.linalg.norm(d, axis=-1, keepdims=True)
    d = d / np.where(norm > 0, norm, 1.0)
    out = {}
    for a, i in enumerate(ids):
        angle = np.degrees(np.arccos(np.clip((d[a][None] * d).sum(-1), -1.0, 1.0)))      # (S, P)
        counts = (seen[a][None] & seen & (angle >= min_angle_deg)).sum(1)
        counts[a] = 0
        order = sorted((j for j in range(len(ids)) if counts[j] > 0), key=lambda j: (-int(counts[j]), ids[j]))
        out[i] = [ids[j] for j in order[:num_sources]]
    return out


def range_rule(depths, percentiles=RANGE_PERCENTILES, widen=RANGE_WIDEN):
    """(near, far) of one image from its sparse depths: the two percentiles of the positive finite depths, near divided
    and far multiplied by `widen` (>= 1; 1.25 leaves room for the surface between and beyond the sparse points)."""
    z = np.asarray(depths, np.float64).reshape(-1)
    z = z[np.isfinite(z) & (z > 0)]
    if len(z) == 0:
        raise ValueError("no positive sparse depth: the image has no depth range")
    if not widen >= 1.0 or not 0.0 <= percentiles[0] <= percentiles[1] <= 100.0:
        raise ValueError("widen must be >= 1 and the percentiles ordered within [0, 100]")
    lo, hi = np.percentile(z, percentiles)
    return float(lo / widen), float(hi * widen)


def depth_ranges(reconstruction, percentiles=RANGE_PERCENTILES, widen=RANGE_WIDEN, device=None):
    """{image name: (near, far)} of every image with sparse depths (dense_depth.sparse_depth on the device, then
    range_rule on the host)."""
    from . import dense_depth as DD

    sd = DD.sparse_depth(reconstruction, device)
    z = sd.uvd[:, 2].cpu().numpy()
    return {name: range_rule(z[int(sd.obs_ptr[k]):int(sd.obs_ptr[k + 1])], percentiles, widen)
            for k, name in enumerate(sd.names)}


# ------------------------------------------------------------------------------------------------ frames -> depth maps
def grey_frames(images):
    """(S,3,H,W) / (1,S,3,H,W) / (S,1,H,W) / (S,H,W) float32 -> (S,H,W) float32 grey = 0.299 R + 0.587 G + 0.114 B."""
    if images.dim() == 5:
        if images.shape[0] != 1:
            raise ValueError("one sequence: images (S,3,H,W) or (1,S,3,H,W)")
        images = images[0]
    if images.dtype != torch.float32:
        raise TypeError(f"images must be float32, got {images.dtype}")
    if images.dim() == 3:
        return images.contiguous()
    if images.dim() != 4 or images.shape[1] not in (1, 3):
        raise ValueError(f"images must be (S,3,H,W), (S,1,H,W) or (S,H,W), got {tuple(images.shape)}")
    if images.shape[1] == 1:
        return images[:, 0].contiguous()
    return (0.299 * images[:, 0] + 0.587 * images[:, 1] + 0.114 * images[:, 2]).contiguous()


def dense_depth_from_frames(reconstruction, images, num_sources=4, min_angle_deg=2.0, num_planes=128, radius=2, min_views=1,
                            min_variance=1e-4, min_conf=0.5, rel_depth_tol=0.01, reproj_tol=1.0, min_consistent=2,
                            range_percentiles=RANGE_PERCENTILES, range_widen=RANGE_WIDEN):
    """Every registered image swept against its source views and checked against their maps.  images: the frames, frame i
    belonging to image id i (as reconstruct_from_frames numbers them), float32 in [0, 1] on the device.  Returns
    (depth_dict, conf_dict) keyed by image name: (H,W) float32 device tensors, depth 0 where there is none (an image without
    source views or sparse depths: all 0).  min_views and min_consistent are capped by the number of sources an image has.
    Raises ValueError when the frames' size is not the cameras', NotImplementedError for camera models other than
    SIMPLE_PINHOLE and SIMPLE_RADIAL."""
    from . import dense_depth as DD

    grey = grey_frames(images)
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
    depth_dict, conf_dict = {}, {}
    if not ids:
        return depth_dict, conf_dict
    row = {i: r for r, i in enumerate(ids)}
    names = [reconstruction.images[i].name for i in ids]
    frames = grey[torch.as_tensor(ids, device=dev)].contiguous()
    poses, cams = torch.from_numpy(pose).to(dev), torch.from_numpy(cam).to(dev)
    rays, ray_index = camera_rays(cam, H, W, dev)
    sources = select_source_views(reconstruction, num_sources, min_angle_deg)
    ranges = depth_ranges(reconstruction, range_percentiles, range_widen, dev)
    raw = torch.zeros(len(ids), H, W, dtype=torch.float32, device=dev)
    for r, i in enumerate(ids):
        src = [row[j] for j in sources[i]]
        conf_dict[names[r]] = torch.zeros(H, W, dtype=torch.float32, device=dev)
        if src and names[r] in ranges:
            near, far = ranges[names[r]]
            sw = plane_sweep(frames, poses, cams, r, src, near, far, num_planes, radius, min(min_views, len(src)), min_variance,
                             min_conf, rays=rays[int(ray_index[r])])
            raw[r], conf_dict[names[r]] = sw.depth, sw.conf
    for r, i in enumerate(ids):
        src = [row[j] for j in sources[i]]
        if src:
            depth_dict[names[r]] = filter_consistent(raw, poses, cams, r, src, rel_depth_tol, reproj_tol,
                                                     min(min_consistent, len(src)), rays, ray_index).depth
        else:
            depth_dict[names[r]] = raw[r].clone()
    return depth_dict, conf_dict


def unproject_depth_maps(reconstruction, depth_dict):
    """{image name: (n,3) float64 device tensor}: the world points of the pixels with depth, row-major inside an image
    (dense_depth.unproject, the kernel of align_dense_depth_maps)."""
    from . import dense_depth as DD

    names = list(depth_dict)
    if not names:
        return {}
    by_name = {reconstruction.images[i].name: i for i in reconstruction.images}
    img_ids = [by_name[n] for n in names]
    packed = DD.pack_maps([depth_dict[n] for n in names], depth_dict[names[0]].device)
    _, cam = DD._camera_rows(reconstruction, img_ids)
    inv = [reconstruction.images[i].cam_from_world.inverse() for i in img_ids]
    inv_pose = np.stack([np.concatenate([t.rotation.matrix(), t.translation[:, None]], axis=1) for t in inv])
    xyz, counts = DD.unproject(packed, packed.flat, cam, inv_pose)
    start = np.concatenate([[0], np.cumsum(counts.cpu().numpy())])
    return {n: xyz[int(start[k]):int(start[k + 1])] for k, n in enumerate(names)}
