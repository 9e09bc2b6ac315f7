"""The last stage of the classical dense path: the depth maps of a reconstruction fused into ONE point cloud -- each
surface point once, with position, normal, colour and the number of views that confirm it -- as HIP kernels
(csrc/fuse/fuse.hip); no namesake in the reference, whose dense output is every depth pixel of every
view unprojected on its own.

    depth_normals               per pixel of every depth map its world-frame normal from the neighbours' points
    fuse_depth_maps             the maps, view by view in a given order -> FusedCloud (de-duplicated, in a fixed order)
    fuse_reconstruction         reconstruction + depth_dict (+ frames) -> FusedCloud, `view` = image id
    write_ply / read_ply        binary little-endian PLY of a cloud (NumPy only)

A point (x, y) with integer coordinates is the centre of pixel [y][x]; depth 0 means "no depth", a normal (0, 0, 0) "no
normal".  What is torch here is plumbing: allocation, the zeroed `claimed` map, the loop over the views (which does not
synchronise with the host) and the final slice to the count."""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib_fuse as F
from ._lib_fuse import check, require_gpu, stream_ptr

_L = F.lib()          # no fallback: importing the fusion without its library is an error

# (below the load: without the library, importing this module fails with lib()'s error whatever else is missing)
from ._dense_args import all_view_inputs, host_i32  # noqa: E402

FusedCloud = namedtuple("FusedCloud", "xyz normal rgb num_views view pixel")

_AUTO = "auto"


def depth_normals(depth, poses, cams, max_rel_jump=0.05, rays=None, ray_index=None):
    """depth (S,H,W) float32 (0: none), poses (S,3,4), cams (S,4) -> (S,H,W,3) float32 on the device: per pixel the unit
    normal of the surface in the world frame, facing its camera, from the central (or one-sided) differences of the
    neighbours' camera-frame points; a neighbour counts when its depth differs by at most max_rel_jump of the pixel's.
    (0, 0, 0) where there is none.  rays (NR,H,W,2) and ray_index (S,): the ray maps and which one a view uses (default:
    mvs.camera_rays(cams)).  What the entry refuses (vggsfm_amd_fuse.h) raises RuntimeError."""
    depth, poses, cams, rays, ridx = all_view_inputs(depth, poses, cams, rays, ray_index)
    S, H, W = depth.shape
    out = torch.empty(S, H, W, 3, dtype=torch.float32, device=depth.device)
    check(_L.vggf_depth_normals(depth, poses, rays, ridx, rays.shape[0], S, H, W, max_rel_jump, out, stream_ptr()),
          "vggf_depth_normals")
    return out


def fuse_depth_maps(depth, poses, cams, sources, colors=None, normals=_AUTO, rel_depth_tol=0.01, reproj_tol=1.0,
                    max_normal_angle_deg=30.0, min_views=2, view_order=None, rays=None, ray_index=None, max_rel_jump=0.05,
                    return_claimed=False):
    """depth (S,H,W) float32 (0: none), poses (S,3,4), cams (S,4), sources: per view the list of its source views (at most
    8, none equal to the view) -> FusedCloud(xyz (N,3) float64, normal (N,3) float32, rgb (N,3) float32, num_views, view,
    pixel (N,) int32) on the device.

    The views are fused in `view_order` (default 0 .. S - 1).  A pixel with depth that no earlier view has claimed is a
    seed; the sources that confirm it forwards and backwards (the test of mvs.filter_consistent, and normals within
    max_normal_angle_deg where both have one) contribute their own world point, normal and colour; with at least
    `min_views` contributors (the seed included) the pixel emits their mean and claims the sources' pixels, which then
    seed nothing themselves.  Points come in the order of the views, row-major inside a view; `pixel` = y W + x of the seed.
    colors: (S,3,H,W) float32 planar, or None: rgb is (N,3) zeros.  normals: "auto" (depth_normals with max_rel_jump), a
    (S,H,W,3) float32 tensor, or None: no normal test and normal is (N,3) zeros.  A view of view_order with fewer than
    min_views - 1 sources is refused, as is everything else the entry refuses (vggsfm_amd_fuse.h): RuntimeError.
    return_claimed: also return the (S,H,W) uint8 map of the claimed pixels."""
    depth, poses, cams, rays, ridx = all_view_inputs(depth, poses, cams, rays, ray_index)
    S, H, W = depth.shape
    dev = depth.device
    if len(sources) != S:
        raise ValueError(f"sources must list the source views of each of the {S} views, got {len(sources)} lists")
    order = list(range(S)) if view_order is None else [int(v) for v in view_order]
    if len(set(order)) != len(order):
        raise ValueError("view_order names a view twice")
    if any(not 0 <= v < S for v in order):
        raise RuntimeError(f"vggf_fuse_view failed: invalid argument (view_order {order} names a view outside [0, {S}))")
    if not 0.0 <= max_normal_angle_deg <= 180.0:
        raise ValueError(f"max_normal_angle_deg must lie in [0, 180], got {max_normal_angle_deg}")
    if isinstance(normals, str):
        if normals != _AUTO:
            raise ValueError(f'normals must be "auto", a tensor or None, got {normals!r}')
        normals = depth_normals(depth, poses, cams, max_rel_jump, rays, ridx)
    if normals is not None:
        if tuple(normals.shape) != (S, H, W, 3) or normals.dtype != torch.float32:
            raise ValueError(f"normals must be {(S, H, W, 3)} float32, got {tuple(normals.shape)} {normals.dtype}")
        normals = normals.contiguous()
        require_gpu(normals)
    if colors is not None:
        if tuple(colors.shape) != (S, 3, H, W) or colors.dtype != torch.float32:
            raise ValueError(f"colors must be {(S, 3, H, W)} float32, got {tuple(colors.shape)} {colors.dtype}")
        colors = colors.contiguous()
        require_gpu(colors)
    src = [host_i32(s) for s in sources]
    plane = H * W
    # a point is a pixel with depth: one host read sizes the outputs
    capacity = int((depth[torch.as_tensor(order, dtype=torch.long, device=dev)] > 0).sum()) if order and plane else 0
    claimed = torch.zeros(S, H, W, dtype=torch.uint8, device=dev)
    counts = torch.zeros(len(order) + 1, dtype=torch.int64, device=dev)
    rows = max(capacity, 1)
    xyz = torch.empty(rows, 3, dtype=torch.float64, device=dev)
    normal = torch.empty(rows, 3, dtype=torch.float32, device=dev) if normals is not None else None
    rgb = torch.empty(rows, 3, dtype=torch.float32, device=dev) if colors is not None else None
    num_views, view, pixel = (torch.empty(rows, dtype=torch.int32, device=dev) for _ in range(3))
    stage_views = torch.empty(max(plane, 1), dtype=torch.int32, device=dev)
    stage_xyz = torch.empty(max(plane, 1), 3, dtype=torch.float64, device=dev)
    stage_normal = torch.empty(max(plane, 1), 3, dtype=torch.float32, device=dev) if normals is not None else None
    stage_rgb = torch.empty(max(plane, 1), 3, dtype=torch.float32, device=dev) if colors is not None else None
    block_counts = torch.empty(max(-(-plane // F.BLOCK), 1), dtype=torch.int32, device=dev)
    cos = math.cos(math.radians(max_normal_angle_deg))
    for k, v in enumerate(order):
        check(_L.vggf_fuse_view(depth, normals, colors, poses, cams, rays, ridx, rays.shape[0], S, H, W, v, src[v], src[v].numel(),
                                rel_depth_tol, reproj_tol, cos, int(min_views), claimed, stage_views, stage_xyz, stage_normal,
                                stage_rgb, block_counts, counts[k:], counts[k + 1:], capacity, xyz, normal, rgb, num_views, view,
                                pixel, stream_ptr()),
              "vggf_fuse_view")
    n = int(counts[-1]) if plane else 0                                    # the one read after the loop
    if n > capacity:
        raise RuntimeError(f"fusion emitted {n} points for {capacity} pixels with depth")
    zeros = lambda: torch.zeros(n, 3, dtype=torch.float32, device=dev)
    cloud = FusedCloud(xyz[:n], normal[:n] if normal is not None else zeros(), rgb[:n] if rgb is not None else zeros(),
                       num_views[:n], view[:n], pixel[:n])
    return (cloud, claimed) if return_claimed else cloud


def fuse_reconstruction(reconstruction, depth_dict, images=None, num_sources=4, min_angle_deg=2.0, **options):
    """The depth maps of a reconstruction (depth_dict by image name, as mvs.dense_depth_from_frames returns it) fused into
    one cloud in the reconstruction's gauge.  Views, poses, cameras, ray maps and source lists are taken as
    dense_depth_from_frames takes them (the registered images in id order, select_source_views); an image without a map
    has no depth, one with fewer than min_views - 1 source views emits nothing.  images: the frames, frame i belonging to
    image id i, (S,3,H,W) / (1,S,3,H,W) float32 colours or (S,1,H,W) / (S,H,W) grey; None: no colours.  `options` are
    fuse_depth_maps' (but view_order: the images are fused in id order).  `view` of the result is the image id."""
    from . import dense_depth as DD
    from . import mvs

    ids = sorted(int(i) for i in reconstruction.reg_image_ids())
    if not ids or not depth_dict:
        raise ValueError("nothing to fuse: no registered image or no depth map")
    first = next(iter(depth_dict.values()))
    require_gpu(first)
    dev = first.device
    H, W = first.shape[-2:]
    names = [reconstruction.images[i].name for i in ids]
    depth = torch.zeros(len(ids), H, W, dtype=torch.float32, device=dev)
    for r, n in enumerate(names):
        if n in depth_dict:
            if tuple(depth_dict[n].shape) != (H, W):
                raise ValueError(f"depth map of {n} is {tuple(depth_dict[n].shape)}, expected {(H, W)}")
            depth[r] = depth_dict[n]
    for i in ids:
        c = reconstruction.cameras[reconstruction.images[i].camera_id]
        if (int(c.height), int(c.width)) != (H, W):
            raise ValueError(f"depth maps are {H} x {W} but the camera of image {i} is {int(c.height)} x {int(c.width)}")
    pose, cam = DD._camera_rows(reconstruction, ids)
    rays, ray_index = mvs.camera_rays(cam, H, W, dev)
    row = {i: r for r, i in enumerate(ids)}
    chosen = mvs.select_source_views(reconstruction, num_sources, min_angle_deg)
    sources = [[row[j] for j in chosen[i]] for i in ids]
    colors = None
    if images is not None:
        frames = images[0] if images.dim() == 5 else images
        if frames.dtype != torch.float32:
            raise TypeError(f"images must be float32, got {frames.dtype}")
        if frames.dim() == 3:
            frames = frames[:, None]
        if frames.dim() != 4 or frames.shape[1] not in (1, 3) or tuple(frames.shape[-2:]) != (H, W):
            raise ValueError(f"images must be (S,3,{H},{W}), (S,1,{H},{W}) or (S,{H},{W}), got {tuple(images.shape)}")
        if max(ids) >= frames.shape[0]:
            raise ValueError(f"image id {max(ids)} has no frame: {frames.shape[0]} frames")
        require_gpu(frames)
        colors = frames[torch.as_tensor(ids, device=dev)].expand(len(ids), 3, H, W).contiguous()
    if "view_order" in options:
        raise ValueError("fuse_reconstruction fuses the registered images in id order; view_order is fuse_depth_maps'")
    # a view with fewer than min_views - 1 sources can emit nothing: it is fused with nobody, and still supports the others
    min_views = int(options.get("min_views", 2))
    order = [r for r in range(len(ids)) if len(sources[r]) + 1 >= min_views]
    cloud = fuse_depth_maps(depth, torch.from_numpy(pose), torch.from_numpy(cam), sources, colors, rays=rays,
                            ray_index=ray_index, view_order=order, **options)
    image_id = torch.as_tensor(ids, dtype=torch.int32, device=dev)[cloud.view.long()]
    return cloud._replace(view=image_id)


# ------------------------------------------------------------------------------------------------------------- PLY
_PLY_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                       ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("num_views", "<i4")])
_PLY_NAMES = {"<f8": "double", "<f4": "float", "|u1": "uchar", "<i4": "int"}


def _host(a, dtype):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a), dtype)


def write_ply(path, cloud):
    """Binary little-endian PLY of a FusedCloud (device or host arrays): x y z double, nx ny nz float, red green blue uchar
    (rgb in [0, 1] x 255, rounded half up and clipped), num_views int; `view` and `pixel` are not stored."""
    xyz, normal, rgb = _host(cloud.xyz, np.float64), _host(cloud.normal, np.float32), _host(cloud.rgb, np.float64)
    n = len(xyz)
    rec = np.empty(n, _PLY_DTYPE)
    rec["x"], rec["y"], rec["z"] = xyz.reshape(n, 3).T
    rec["nx"], rec["ny"], rec["nz"] = normal.reshape(n, 3).T
    rec["red"], rec["green"], rec["blue"] = np.clip(np.floor(rgb.reshape(n, 3) * 255.0 + 0.5), 0, 255).astype(np.uint8).T
    rec["num_views"] = _host(cloud.num_views, np.int32)
    props = "".join(f"property {_PLY_NAMES[_PLY_DTYPE[name].str]} {name}\n" for name in _PLY_DTYPE.names)
    with open(path, "wb") as f:
        f.write(f"ply\nformat binary_little_endian 1.0\nelement vertex {n}\n{props}end_header\n".encode("ascii"))
        f.write(rec.tobytes())


def read_ply(path):
    """The FusedCloud of a file written by write_ply, as NumPy arrays: rgb back in [0, 1] (uchar / 255, float32); `view` and
    `pixel`, which the file does not hold, are -1."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").split("\n")
    if header[0] != "ply" or header[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    n = int(next(line for line in header if line.startswith("element vertex ")).split()[2])
    props = [tuple(line.split()[1:]) for line in header if line.startswith("property ")]
    if props != [(_PLY_NAMES[_PLY_DTYPE[name].str], name) for name in _PLY_DTYPE.names]:
        raise ValueError(f"{path}: not the properties write_ply writes: {props}")
    rec = np.frombuffer(data, _PLY_DTYPE, count=n, offset=end)
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], -1).astype(np.float64).reshape(n, 3)
    normal = np.stack([rec["nx"], rec["ny"], rec["nz"]], -1).astype(np.float32).reshape(n, 3)
    rgb = (np.stack([rec["red"], rec["green"], rec["blue"]], -1).astype(np.float32) / np.float32(255.0)).reshape(n, 3)
    none = np.full(n, -1, np.int32)
    return FusedCloud(xyz, normal, rgb, rec["num_views"].astype(np.int32), none, none.copy())
