"""Reprojection video on the MI355X: the reference's ``make_reproj_video`` stage (vggsfm/runners/runner.py:834-885,
vggsfm/utils/utils.py:393-571) over ``vgg_reproj_stats`` / ``vgg_reproj_visible`` / ``vgg_reproj_draw``
(vggsfm_amd/csrc/reproj.hip).

* :func:`render` -- every frame of the video as a padded BGR canvas on the device: colour statistics over all points,
  per observation its rounded centre, colormap colour and whether it wins its pixel (smallest depth), then the winning
  circles composited onto the frame.  Frames are processed in chunks so that the per-frame visibility grids stay bounded.
* :func:`filter_mask` -- the standalone visibility mask of ``filter_invisible_reprojections`` on the same kernels.

Circles follow an integer raster rule (4 x 4 sub-samples per pixel) in place of OpenCV's
anti-aliased fill; everything else -- statistics, centres, colours, the visible set and the drawing order -- is the
reference's exactly.  There is no CPU path.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib

COLOR_MODES = {"dis_to_center": 0, "dis_to_origin": 1, "point_order": 2}
MAX_RADIUS = 32                 # VGG_REPROJ_MAX_RADIUS of include/vggsfm_amd.h
MAX_GRID_CELLS = 1 << 25        # cells of one chunk of visibility grids (12 B each: ~400 MB)
FILTER_MAX_CELLS = 1 << 27      # bounding-box cells of the standalone mask (filter_mask)

Debug = namedtuple("Debug", "names obs_range visible centers colors stats")


def _dev(device):
    return torch.device("cuda" if device is None else device)


def _to_dev(a, dtype, dev):
    """A host array as a contiguous device tensor of `dtype` (a numpy dtype)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def colormap_lut(cmap):
    """(N + 3, 3) int64 table of ``(Colormap(x)[:3] * 255).astype(int)``: the N colours, then under, over and bad (the
    layout of matplotlib's ``Colormap._lut``).  `cmap`: a name (resolved with matplotlib), a ``Colormap`` or an (N + 3, 4)
    / (N + 3, 3) float array of such a ``_lut``."""
    if isinstance(cmap, str) or hasattr(cmap, "_lut") or hasattr(cmap, "_init"):
        if isinstance(cmap, str):
            import matplotlib
            cmap = matplotlib.colormaps.get_cmap(cmap)
        if not cmap._isinit:
            cmap._init()
        lut = np.asarray(cmap._lut, np.float64)
    else:
        lut = np.asarray(cmap, np.float64)
    if lut.ndim != 2 or lut.shape[1] not in (3, 4) or lut.shape[0] < 4:
        raise ValueError(f"cmap: expected a colormap or an (N + 3, 4) lookup table, got shape {lut.shape}")
    return (lut[:, :3] * 255).astype(int)


def pack_lut(lut_int):
    """(N + 3, 3) ints in 0..255 -> (N + 3,) uint32 r | g << 8 | b << 16, N."""
    c = np.asarray(lut_int, np.int64)
    if c.min() < 0 or c.max() > 255:
        raise ValueError("cmap: colours must lie in [0, 1]")
    return (c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16)).astype(np.uint32), len(c) - 3


def live_points(reconstruction):
    """(xyz (P,3) float64, point ids (P,) int64) of all points of the model (``reconstruction.points3D``)."""
    if hasattr(reconstruction, "_alive") and hasattr(reconstruction, "_xyz"):
        ids = np.nonzero(reconstruction._alive[:reconstruction._n])[0]
        return np.ascontiguousarray(reconstruction._xyz[ids], np.float64), (ids + 1).astype(np.int64)
    pts = reconstruction.points3D
    ids = np.array(list(pts.keys()), np.int64)
    xyz = np.array([pts[i].xyz for i in ids], np.float64).reshape(-1, 3)
    return xyz, ids


def stats(points3D, point_ids, color_mode, device=None):
    """Colour statistics (8,) float64 on the device (layout: include/vggsfm_amd.h, vgg_reproj_stats)."""
    L = _lib.lib()
    dev = _dev(device)
    mode = COLOR_MODES[color_mode]
    xyz = torch.as_tensor(points3D).to(device=dev, dtype=torch.float64).reshape(-1, 3).contiguous()
    ids = torch.as_tensor(point_ids).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    P = xyz.shape[0] if mode != 2 else ids.shape[0]
    if P == 0:
        raise ValueError("the reconstruction has no 3D points: the colour statistics are undefined")
    out = torch.zeros(8, dtype=torch.float64, device=dev)
    nbytes = L.vgg_reproj_stats_workspace_bytes(P)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(L.vgg_reproj_stats(xyz if mode != 2 else None, ids if mode == 2 else None, P, mode, out, ws, nbytes,
                                  _lib.stream_ptr()), "vgg_reproj_stats")
    return out


def _chunks(cells, budget):
    """[(begin, end)] frame ranges whose grid cells stay within `budget` (a frame larger than it gets a chunk of its own)."""
    out, b, acc = [], 0, 0
    for f, c in enumerate(cells):
        if f > b and acc + c > budget:
            out.append((b, f))
            b, acc = f, 0
        acc += c
    if b < len(cells):
        out.append((b, len(cells)))
    return out


def _validate(images, video_size, draw_radius, color_mode):
    if color_mode not in COLOR_MODES:
        raise NotImplementedError(f"Color mode '{color_mode}' is not implemented.")
    if int(draw_radius) != draw_radius or draw_radius < 0:
        raise ValueError(f"draw_radius must be a non-negative integer, got {draw_radius}")
    if draw_radius > MAX_RADIUS:
        raise ValueError(f"draw_radius {draw_radius} exceeds the supported maximum {MAX_RADIUS}")
    W, H = int(video_size[0]), int(video_size[1])
    if W <= 0 or H <= 0:
        raise ValueError(f"video_size must be positive (width, height), got {tuple(video_size)}")
    for name, im in images.items():
        shp = tuple(im.shape)
        if len(shp) != 3 or shp[2] != 3:
            raise ValueError(f"image {name!r}: expected (H, W, 3) RGB, got shape {shp}")
        if im.dtype not in (np.uint8, torch.uint8):
            raise ValueError(f"image {name!r}: expected uint8, got {im.dtype}")
        if shp[0] > H or shp[1] > W:
            raise ValueError(f"image {name!r} ({shp[1]} x {shp[0]}) is larger than the video ({W} x {H})")
    return W, H


def render(sparse_depth_device, points3D, point_ids, images, video_size, draw_radius=3, cmap="gist_rainbow",
           color_mode="dis_to_center", device=None, return_debug=False, max_grid_cells=MAX_GRID_CELLS):
    """The video frames as one (S, H, W, 3) uint8 BGR device tensor, frames in ``sorted(images)`` order.

    sparse_depth_device: :class:`vggsfm_amd.dense_depth.SparseDepth` (names, obs_ptr, uvd (O,3), xyzid (O,4) on the
    device), as ``GeometryRunner.extract_sparse_depth_and_point_from_reconstruction`` leaves it.  points3D (P,3) / point_ids
    (P,): all points of the model (the colour statistics).  images: {name: (h, w, 3) uint8 RGB}, numpy or device tensors,
    h <= H and w <= W; a name without observations is output undrawn.  video_size: (W, H).  With `return_debug` also a
    :class:`Debug` (per observation: visible uint8, centers (O,2) int32 (INT32_MIN off the window), colors (O,3) uint8;
    stats (8,) float64; obs_range (S,2) of each frame)."""
    W, H = _validate(images, video_size, draw_radius, color_mode)
    r = int(draw_radius)
    mode = COLOR_MODES[color_mode]
    lut_u32, N = pack_lut(colormap_lut(cmap))
    L = _lib.lib()
    dev = _dev(device)
    sd = sparse_depth_device
    names = sorted(images)
    S = len(names)
    O = int(sd.obs_ptr[-1])
    if O >= 2 ** 31 - 1:
        raise ValueError(f"{O} observations: at most 2^31 - 2 are supported")
    slot = {n: k for k, n in enumerate(sd.names)}
    obs_range = np.zeros((S, 2), np.int64)
    for f, n in enumerate(names):
        if n in slot:
            obs_range[f] = sd.obs_ptr[slot[n]], sd.obs_ptr[slot[n] + 1]
    hw = np.array([tuple(images[n].shape[:2]) for n in names], np.int64).reshape(-1, 2)
    cells = (hw[:, 0] + 2 * r) * (hw[:, 1] + 2 * r)
    grid_off = np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)
    counts = obs_range[:, 1] - obs_range[:, 0]
    img_sizes = hw[:, 0] * hw[:, 1] * 3
    img_off = np.concatenate([[0], np.cumsum(img_sizes)]).astype(np.int64)

    T = lambda a, dt: _to_dev(a, dt, dev)
    st = stats(points3D, point_ids, color_mode, dev)
    flat = torch.cat([torch.as_tensor(images[n]).to(dev).reshape(-1) for n in names]) if S else \
        torch.zeros(0, dtype=torch.uint8, device=dev)
    flat = flat.contiguous()
    range_t, h_t, w_t = T(obs_range, np.int64), T(hw[:, 0], np.int32), T(hw[:, 1], np.int32)
    goff_t, ioff_t, lut_t = T(grid_off, np.int64), T(img_off, np.int64), T(lut_u32.view(np.int32), np.int32)
    obs_cell = torch.empty(max(O, 1), dtype=torch.int32, device=dev)
    color = torch.zeros(max(O, 1), dtype=torch.int32, device=dev)
    centers = torch.full((max(O, 1), 2), -2 ** 31, dtype=torch.int32, device=dev) if return_debug else None
    visible = torch.zeros(max(O, 1), dtype=torch.uint8, device=dev) if return_debug else None
    out = torch.empty((S, H, W, 3), dtype=torch.uint8, device=dev)
    chunks = _chunks(cells, max_grid_cells)
    max_cells = max([int(grid_off[e] - grid_off[b]) for b, e in chunks] + [1])
    if max_cells > 2 ** 31 - 1:
        raise ValueError(f"a frame of {max_cells} grid cells is too large (at most 2^31 - 1)")
    grid_key = torch.empty(max_cells, dtype=torch.int64, device=dev)
    grid_obs = torch.empty(max_cells, dtype=torch.int32, device=dev)
    for b, e in chunks:
        _lib.check(L.vgg_reproj_visible(sd.uvd, sd.xyzid, range_t, h_t, w_t, goff_t, b, e, counts[b:e].max(),
                                        grid_off[e] - grid_off[b], r, mode, st, lut_t, N, obs_cell, color, centers, visible,
                                        grid_key, grid_obs, _lib.stream_ptr()), "vgg_reproj_visible")
        _lib.check(L.vgg_reproj_draw(flat, ioff_t, h_t, w_t, goff_t, b, e, H, W, r, grid_obs, color, out[b:e],
                                     _lib.stream_ptr()), "vgg_reproj_draw")
    if not return_debug:
        return out
    c = color[:O].to(torch.int64)
    colors = torch.stack([c & 255, (c >> 8) & 255, (c >> 16) & 255], dim=1).to(torch.uint8)
    return out, Debug(names, obs_range, visible[:O], centers[:O], colors, st)


def filter_mask(uvs_int, depths, max_cells=FILTER_MAX_CELLS):
    """``filter_invisible_reprojections`` (utils.py:393-425): True for the observations that win their integer pixel
    (smallest depth; ties to the lowest index; -0.0 == +0.0; a NaN depth first).  uvs_int (n,2) integers and depths (n,),
    numpy or device tensors; numpy in -> numpy bool out, device in -> device bool out.  The grid is the bounding box of the
    points; one of more than `max_cells` cells raises ValueError (the reference has no such limit)."""
    on_device = torch.is_tensor(uvs_int) and uvs_int.is_cuda
    dev = uvs_int.device if on_device else _dev(None)
    uv = torch.as_tensor(uvs_int).to(dev)
    if uv.ndim != 2 or uv.shape[1] != 2:
        raise ValueError(f"uvs_int must be (n, 2), got shape {tuple(uv.shape)}")
    if uv.dtype.is_floating_point or uv.dtype == torch.bool:
        raise ValueError(f"uvs_int must be integer, got {uv.dtype}")
    n = uv.shape[0]
    d = torch.as_tensor(depths).to(dev).reshape(-1)
    if d.shape[0] != n:
        raise ValueError(f"{d.shape[0]} depths for {n} points")
    if n == 0:
        m = torch.ones(0, dtype=torch.bool, device=dev)
        return m if on_device else m.cpu().numpy()
    if n >= 2 ** 31 - 1:
        raise ValueError(f"{n} points: at most 2^31 - 2 are supported")
    uv = uv.to(torch.int64)
    lo = uv.min(dim=0).values
    ext = (uv.max(dim=0).values - lo + 1).cpu().numpy()
    w, h = int(ext[0]), int(ext[1])
    if w <= 0 or h <= 0 or w * h > max_cells:
        raise ValueError(f"filter_invisible_reprojections: the points span {w} x {h} = {w * h} pixels, more than the "
                         f"{max_cells} the device grid supports")
    uvd = torch.stack([(uv[:, 0] - lo[0]).double(), (uv[:, 1] - lo[1]).double(), d.double()], dim=1).contiguous()
    L = _lib.lib()
    T = lambda a, dt: _to_dev(a, dt, dev)
    obs_cell = torch.empty(n, dtype=torch.int32, device=dev)
    visible = torch.empty(n, dtype=torch.uint8, device=dev)
    grid_key = torch.empty(w * h, dtype=torch.int64, device=dev)
    grid_obs = torch.empty(w * h, dtype=torch.int32, device=dev)
    rng, h_t, w_t, goff = T([[0, n]], np.int64), T([h], np.int32), T([w], np.int32), T([0, w * h], np.int64)
    _lib.check(L.vgg_reproj_visible(uvd, None, rng, h_t, w_t, goff, 0, 1, n, w * h, 0, 0, None, None, 0, obs_cell, None, None,
                                    visible, grid_key, grid_obs, _lib.stream_ptr()), "vgg_reproj_visible")
    m = visible.bool()
    return m if on_device else m.cpu().numpy()
