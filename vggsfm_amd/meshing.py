"""The surface of the classical dense path: the depth maps of a reconstruction integrated into a truncated signed distance
(TSDF) volume and the zero level set of that volume extracted as an indexed triangle mesh by marching tetrahedra on the
Kuhn split of each cell, as HIP kernels (csrc/tsdf/tsdf.hip); no namesake in the reference, whose
users mesh elsewhere.

    TSDFVolume                  the volume on the device: .integrate(depth maps) any number of times, .extract() -> Mesh
    volume_bounds               a grid around a point set (1st to 99th percentile box, grown by a margin)
    mesh_reconstruction         reconstruction + depth_dict (+ frames, + confidences) -> Mesh
    write_mesh_ply / read_mesh_ply   binary little-endian PLY of a mesh (NumPy only)

The mesh is watertight wherever the volume has been observed (the split is translation invariant, so neighbouring cells agree
on every face diagonal), its triangles and vertex normals point to growing distance, which is towards the cameras, and its
vertices and faces come in a fixed order (by node, by cell): two runs give the same bits.  What is torch here is plumbing:
allocation, the zeroed volumes, the one read of the two counts between counting and emission, and volume_bounds."""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib_tsdf as T
from ._lib_tsdf import check, require_gpu, stream_ptr
from ._dense_args import f64, maps
from .fusion import _PLY_NAMES, _host

_L = T.lib()          # no fallback: importing the meshing without its library is an error

Mesh = namedtuple("Mesh", "vertices normals rgb faces")


def case_table():
    """The kernel's 16-case table as vggv_case_table returns it: (2, 16, 7) int32 NumPy array."""
    out = torch.empty(2, 16, 7, dtype=torch.int32)
    check(_L.vggv_case_table(out), "vggv_case_table")
    return out.numpy().copy()


def _check_grid(voxel, dims):
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3 or min(dims) < 2:
        raise ValueError(f"dims must be three numbers of nodes, each >= 2, got {dims}")
    if dims[0] * dims[1] * dims[2] > T.MAX_NODES:
        raise ValueError(f"a grid of {dims[0]} x {dims[1]} x {dims[2]} nodes is too large: at most {T.MAX_NODES} nodes")
    if not float(voxel) > 0.0:
        raise ValueError(f"voxel must be > 0, got {voxel}")
    return dims


class TSDFVolume:
    """A regular grid of nx x ny x nz nodes, node (i, j, k) at origin + voxel (i, j, k), holding per node the weighted sums
    of the truncated signed distances, of the weights and (color=True) of the colours of every depth map integrated so far,
    as float64 device tensors tsdf_sum (N), weight_sum (N), rgb_sum (N, 3) with N = nx ny nz and n = (k ny + j) nx + i."""

    def __init__(self, origin, voxel, dims, color=True, device="cuda"):
        self.dims = _check_grid(voxel, dims)
        self.voxel = float(voxel)
        self.origin = tuple(float(o) for o in np.asarray(origin, dtype=np.float64).reshape(3))
        if not all(math.isfinite(o) for o in self.origin):
            raise ValueError(f"origin must be finite, got {self.origin}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("vggsfm_amd kernels need tensors on an MI355X (cuda) device; there is no CPU path")
        N = self.dims[0] * self.dims[1] * self.dims[2]
        self.tsdf_sum = torch.zeros(N, dtype=torch.float64, device=dev)
        self.weight_sum = torch.zeros(N, dtype=torch.float64, device=dev)
        self.rgb_sum = torch.zeros(N, 3, dtype=torch.float64, device=dev) if color else None

    @property
    def num_nodes(self):
        return self.tsdf_sum.numel()

    def integrate(self, depth, poses, cams, weights=None, frames=None, trunc=None):
        """depth (S,H,W) float32 (0: none), poses (S,3,4) [R|t] camera from world, cams (S,4) f, cx, cy, k: the views are
        integrated in order onto the volume's contents.  Per node and view: the node is projected to its nearest pixel; with
        z the depth there and zc the node's own depth, sdf = z - zc; a node further than `trunc` BEHIND the surface is left
        alone, else min(1, sdf / trunc) is added with the pixel's weight.  weights (S,H,W) float32 or None (1); a pixel
        with weight 0 adds nothing.  frames (S,3,H,W) float32 planar colours or None (a volume with colour then keeps what
        it has).  trunc defaults to 4 voxels -- a default, not a tuned value: it must exceed the noise of the maps and
        stay below the thinnest structure.  Returns self."""
        depth = maps(depth, "depth")
        S, H, W = depth.shape
        if S < 1:
            raise ValueError("no view to integrate")
        dev = self.tsdf_sum.device
        poses, cams = f64(poses, (S, 3, 4), "poses").to(dev), f64(cams, (S, 4), "cams").to(dev)
        trunc = 4.0 * self.voxel if trunc is None else float(trunc)
        if not trunc > 0.0:
            raise ValueError(f"trunc must be > 0, got {trunc}")
        for name, t, shape in (("weights", weights, (S, H, W)), ("frames", frames, (S, 3, H, W))):
            if t is not None:
                if tuple(t.shape) != shape or t.dtype != torch.float32:
                    raise ValueError(f"{name} must be {shape} float32, got {tuple(t.shape)} {t.dtype}")
                require_gpu(t)
        weights = None if weights is None else weights.contiguous()
        frames = None if frames is None or self.rgb_sum is None else frames.contiguous()
        check(_L.vggv_integrate(depth, weights, frames, poses, cams, S, H, W, *self.origin, self.voxel, *self.dims, trunc,
                                self.tsdf_sum, self.weight_sum, self.rgb_sum if frames is not None else None, stream_ptr()),
              "vggv_integrate")
        return self

    def count(self, min_weight=1.0):
        """The counting half of extract(): -> dict of device tensors edge_mask (N) uint8, vertex_offset, face_offset (N) int32,
        group_counts (G,2) int32, group_offsets (G,2) int64, counts (2) int64 = (V, F) (vggsfm_amd_tsdf.h)."""
        if not float(min_weight) > 0.0:
            raise ValueError(f"min_weight must be > 0, got {min_weight}")
        dev, N = self.tsdf_sum.device, self.num_nodes
        G = -(-N // T.GROUP)
        out = {"edge_mask": torch.empty(N, dtype=torch.uint8, device=dev),
               "vertex_offset": torch.empty(N, dtype=torch.int32, device=dev),
               "face_offset": torch.empty(N, dtype=torch.int32, device=dev),
               "group_counts": torch.empty(G, 2, dtype=torch.int32, device=dev),
               "group_offsets": torch.empty(G, 2, dtype=torch.int64, device=dev),
               "counts": torch.empty(2, dtype=torch.int64, device=dev)}
        check(_L.vggv_mesh_count(self.tsdf_sum, self.weight_sum, *self.dims, float(min_weight), out["edge_mask"],
                                 out["vertex_offset"], out["face_offset"], out["group_counts"], out["group_offsets"],
                                 out["counts"], stream_ptr()), "vggv_mesh_count")
        return out

    def emit(self, count, num_vertices, num_faces, min_weight=1.0):
        """The emission half of extract(): the Mesh of `count` (of .count() with the same min_weight) with room for
        num_vertices and num_faces rows."""
        dev = self.tsdf_sum.device
        V, F = int(num_vertices), int(num_faces)
        vertices = torch.empty(max(V, 1), 3, dtype=torch.float64, device=dev)
        normals = torch.empty(max(V, 1), 3, dtype=torch.float32, device=dev)
        rgb = torch.empty(max(V, 1), 3, dtype=torch.float32, device=dev) if self.rgb_sum is not None else None
        faces = torch.empty(max(F, 1), 3, dtype=torch.int32, device=dev)
        check(_L.vggv_mesh_emit(self.tsdf_sum, self.weight_sum, self.rgb_sum, *self.origin, self.voxel, *self.dims,
                                float(min_weight), count["edge_mask"], count["vertex_offset"], count["face_offset"],
                                count["group_offsets"], V, F, vertices, normals, rgb, faces, stream_ptr()), "vggv_mesh_emit")
        rgb = rgb[:V] if rgb is not None else torch.zeros(V, 3, dtype=torch.float32, device=dev)
        return Mesh(vertices[:V], normals[:V], rgb, faces[:F])

    def extract(self, min_weight=1.0):
        """The zero level set over the nodes with weight_sum >= min_weight -> Mesh(vertices (V,3) float64, normals (V,3)
        float32 (unit, towards growing distance; (0,0,0) where the volume gives none), rgb (V,3) float32 (zeros without
        colour), faces (F,3) int32 rows of `vertices`) on the device.  One host read, of the two counts, sizes the outputs."""
        count = self.count(min_weight)
        V, F = (int(c) for c in count["counts"].tolist())                       # the one read between counting and emission
        return self.emit(count, V, F, min_weight)


def volume_bounds(points, resolution=256, margin=0.05):
    """A grid for a point set (P,3) on the device: the box from the 1st to the 99th percentile of every coordinate, grown on
    every side by `margin` x its longest side, with `resolution` nodes along that longest side -> (origin (3 floats), voxel,
    dims (nx, ny, nz)), each dim >= 2.  Runs in torch on the points' device."""
    points = torch.as_tensor(points)
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError(f"points must be (P,3) with P >= 1, got {tuple(points.shape)}")
    if int(resolution) < 2:
        raise ValueError(f"resolution must be >= 2, got {resolution}")
    if not float(margin) >= 0.0:
        raise ValueError(f"margin must be >= 0, got {margin}")
    p = points.to(torch.float64)
    p = p[torch.isfinite(p).all(1)]
    if p.shape[0] < 1:
        raise ValueError("no finite point")
    srt = torch.sort(p, 0).values
    P = srt.shape[0]
    lo, hi = srt[int(math.floor(0.01 * (P - 1)))], srt[int(math.ceil(0.99 * (P - 1)))]
    lo, hi = lo.tolist(), hi.tolist()
    side = max(h - l for l, h in zip(lo, hi))
    if not side > 0.0:
        raise ValueError("the points span no volume")
    grow = float(margin) * side
    lo, hi = [l - grow for l in lo], [h + grow for h in hi]
    voxel = (side + 2.0 * grow) / (int(resolution) - 1)
    dims = tuple(max(2, int(math.ceil((h - l) / voxel - 1e-9)) + 1) for l, h in zip(lo, hi))
    return tuple(lo), voxel, dims


def mesh_reconstruction(reconstruction, depth_dict, images=None, conf_dict=None, resolution=256, margin=0.05, trunc=None,
                        min_weight=1.0, bounds=None):
    """The depth maps of a reconstruction (depth_dict by image name, as mvs.dense_depth_from_frames returns it) meshed in the
    reconstruction's gauge.  Views, poses and cameras are taken as fusion.fuse_reconstruction takes them (the registered
    images in id order; an image without a map has no depth).  images: the frames, frame i belonging to image id i,
    (S,3,H,W) / (1,S,3,H,W) float32 colours or (S,1,H,W) / (S,H,W) grey; None: no colours.  conf_dict: per image name an
    (H,W) float32 weight map (an image without one weighs 1); None: every weight 1.  bounds: (origin, voxel, dims), default
    volume_bounds(the maps' points, every 4th pixel, resolution, margin).  trunc: TSDFVolume.integrate's (4 voxels by
    default); min_weight: TSDFVolume.extract's.  -> Mesh."""
    from . import dense_depth as DD

    ids = sorted(int(i) for i in reconstruction.reg_image_ids())
    if not ids or not depth_dict:
        raise ValueError("nothing to mesh: no registered image or no depth map")
    first = next(iter(depth_dict.values()))
    require_gpu(first)
    dev = first.device
    H, W = first.shape[-2:]
    names = [reconstruction.images[i].name for i in ids]
    S = len(ids)
    depth = torch.zeros(S, H, W, dtype=torch.float32, device=dev)
    weights = None if conf_dict is None else torch.ones(S, H, W, dtype=torch.float32, device=dev)
    for r, n in enumerate(names):
        if n in depth_dict:
            if tuple(depth_dict[n].shape) != (H, W):
                raise ValueError(f"depth map of {n} is {tuple(depth_dict[n].shape)}, expected {(H, W)}")
            depth[r] = depth_dict[n]
        if conf_dict is not None and n in conf_dict:
            if tuple(conf_dict[n].shape) != (H, W):
                raise ValueError(f"weight map of {n} is {tuple(conf_dict[n].shape)}, expected {(H, W)}")
            weights[r] = conf_dict[n]
    for i in ids:
        c = reconstruction.cameras[reconstruction.images[i].camera_id]
        if (int(c.height), int(c.width)) != (H, W):
            raise ValueError(f"depth maps are {H} x {W} but the camera of image {i} is {int(c.height)} x {int(c.width)}")
    pose, cam = DD._camera_rows(reconstruction, ids)
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
        colors = frames[torch.as_tensor(ids, device=dev)].expand(S, 3, H, W).contiguous()
    poses_t, cams_t = torch.from_numpy(pose).to(dev), torch.from_numpy(cam).to(dev)
    if bounds is None:
        bounds = volume_bounds(_depth_points(depth, poses_t, cams_t, 4), resolution, margin)
    origin, voxel, dims = bounds
    volume = TSDFVolume(origin, voxel, dims, color=colors is not None, device=dev)
    volume.integrate(depth, poses_t, cams_t, weights, colors, trunc)
    return volume.extract(min_weight)


def _depth_points(depth, poses, cams, stride):
    """world points (P,3) float64 of every `stride`-th pixel with depth, in torch (for volume_bounds only)"""
    from .mvs import camera_rays

    S, H, W = depth.shape
    rays, ray_index = camera_rays(cams, H, W, depth.device)
    out = []
    for s in range(S):
        z = depth[s, ::stride, ::stride].to(torch.float64)
        ray = rays[int(ray_index[s])][::stride, ::stride]
        keep = z > 0
        P = torch.stack([ray[..., 0] * z, ray[..., 1] * z, z], -1)[keep]
        R, t = poses[s, :, :3], poses[s, :, 3]
        out.append((P - t) @ R)                                              # R^T (P - t)
    pts = torch.cat(out)
    if pts.shape[0] < 1:
        raise ValueError("nothing to mesh: no pixel with depth")
    return pts


# ------------------------------------------------------------------------------------------------------------- PLY
_VERTEX_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                          ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("num_views", "<i4")])
_FACE_DTYPE = np.dtype([("count", "u1"), ("v", "<i4", (3,))])
_FACE_LINE = "property list uchar int vertex_indices"


def write_mesh_ply(path, mesh):
    """Binary little-endian PLY of a Mesh (device or host arrays): the vertex properties of fusion.write_ply -- x y z double,
    nx ny nz float, red green blue uchar (rgb in [0, 1] x 255, rounded half up and clipped), num_views int (0: a mesh
    vertex has none) -- and `element face` as `property list uchar int vertex_indices`."""
    xyz, normal, rgb = _host(mesh.vertices, np.float64), _host(mesh.normals, np.float32), _host(mesh.rgb, np.float64)
    faces = _host(mesh.faces, np.int32).reshape(-1, 3)
    n = len(xyz)
    rec = np.zeros(n, _VERTEX_DTYPE)
    rec["x"], rec["y"], rec["z"] = xyz.reshape(n, 3).T
    rec["nx"], rec["ny"], rec["nz"] = normal.reshape(n, 3).T
    rec["red"], rec["green"], rec["blue"] = np.clip(np.floor(rgb.reshape(n, 3) * 255.0 + 0.5), 0, 255).astype(np.uint8).T
    frec = np.zeros(len(faces), _FACE_DTYPE)
    frec["count"], frec["v"] = 3, faces
    props = "".join(f"property {_PLY_NAMES[_VERTEX_DTYPE[name].str]} {name}\n" for name in _VERTEX_DTYPE.names)
    with open(path, "wb") as f:
        f.write(f"ply\nformat binary_little_endian 1.0\nelement vertex {n}\n{props}element face {len(faces)}\n{_FACE_LINE}\n"
                "end_header\n".encode("ascii"))
        f.write(rec.tobytes())
        f.write(frec.tobytes())


def read_mesh_ply(path):
    """The Mesh of a file written by write_mesh_ply, as NumPy arrays: rgb back in [0, 1] (uchar / 255, float32).  Any other
    header raises ValueError."""
    with open(path, "rb") as f:
        data = f.read()
    mark = data.find(b"end_header\n")
    if mark < 0:
        raise ValueError(f"{path}: not a PLY file: no end_header")
    end = mark + len(b"end_header\n")
    try:
        header = data[:end].decode("ascii").split("\n")
    except UnicodeDecodeError:
        raise ValueError(f"{path}: not a PLY header") from None
    if len(header) < 3 or header[0] != "ply" or header[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    want = ["ply", "format binary_little_endian 1.0", "element vertex"] + \
        [f"property {_PLY_NAMES[_VERTEX_DTYPE[name].str]} {name}" for name in _VERTEX_DTYPE.names] + \
        ["element face", _FACE_LINE, "end_header", ""]
    counts = []
    if len(header) != len(want):
        raise ValueError(f"{path}: not the header write_mesh_ply writes: {header}")
    for line, w in zip(header, want):
        if w.startswith("element "):
            parts = line.split()
            if len(parts) != 3 or " ".join(parts[:2]) != w or not parts[2].isdigit():
                raise ValueError(f"{path}: not the header write_mesh_ply writes: {line!r}")
            counts.append(int(parts[2]))
        elif line != w:
            raise ValueError(f"{path}: not the header write_mesh_ply writes: {line!r}")
    n, m = counts
    if len(data) != end + n * _VERTEX_DTYPE.itemsize + m * _FACE_DTYPE.itemsize:
        raise ValueError(f"{path}: {len(data) - end} bytes of data for {n} vertices and {m} faces")
    rec = np.frombuffer(data, _VERTEX_DTYPE, count=n, offset=end)
    frec = np.frombuffer(data, _FACE_DTYPE, count=m, offset=end + n * _VERTEX_DTYPE.itemsize)
    if m and (frec["count"] != 3).any():
        raise ValueError(f"{path}: a face that is no triangle")
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], -1).astype(np.float64).reshape(n, 3)
    normal = np.stack([rec["nx"], rec["ny"], rec["nz"]], -1).astype(np.float32).reshape(n, 3)
    rgb = (np.stack([rec["red"], rec["green"], rec["blue"]], -1).astype(np.float32) / np.float32(255.0)).reshape(n, 3)
    return Mesh(xyz, normal, rgb, frec["v"].astype(np.int32).reshape(m, 3))
