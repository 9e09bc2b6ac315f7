"""The dense mesh seen from the cameras: a z-buffer rasteriser that draws a triangle mesh into the views of a
reconstruction and gives, per view and pixel, the depth of the nearest face, that face, and the mesh's normals and colours
interpolated on it, as HIP kernels (csrc/raster/raster.hip); no namesake in the reference, whose
users render elsewhere.

    new_keys / rasterize / resolve   the two halves: faces drawn onto a buffer of 64-bit keys, the buffer resolved to maps
    render_mesh                      a meshing.Mesh (or bare tensors) + cameras -> Rendered
    visible_points                   which 3D points a depth map does not occlude, per view
    render_reconstruction            reconstruction + mesh -> depth, normal, colour and face maps by image name

A key is (the float32 depth's bits) << 32 | the face's index and a pixel keeps the smallest key drawn onto it, so the maps do
not depend on the order of the faces, on how they are split over calls or on how the kernel spreads its work: two runs give
the same bits, and several meshes may be drawn into one buffer.  Depth maps are hole-free wherever the mesh is, and
occlusion-correct.  What is torch here is plumbing: allocation, the cleared key buffer and the default ray maps."""
from collections import namedtuple

import torch

from . import _lib_raster as Z
from ._lib_raster import check, require_gpu, stream_ptr
from ._dense_args import f64, host_i32

_L = Z.lib()          # no fallback: importing the renderer without its library is an error

Rendered = namedtuple("Rendered", "depth face normal rgb weights")


def new_keys(S, H, W, device="cuda"):
    """The cleared key buffer of S views of H x W pixels: an int64 device tensor filled with -1 (all ones = empty)."""
    S, H, W = int(S), int(H), int(W)
    if S < 1 or H < 0 or W < 0:
        raise ValueError(f"keys need S >= 1 views of H, W >= 0 pixels, got {(S, H, W)}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("vggsfm_amd kernels need tensors on an MI355X (cuda) device; there is no CPU path")
    return torch.full((S, H, W), -1, dtype=torch.int64, device=dev)


def _keys(keys):
    if not torch.is_tensor(keys) or keys.dim() != 3 or keys.dtype != torch.int64 or not keys.is_contiguous():
        raise ValueError("keys must be a contiguous (S,H,W) int64 tensor (new_keys)")
    require_gpu(keys)
    if keys.shape[0] < 1:
        raise ValueError("keys without a view")
    return keys


def _mesh(vertices, faces, dev):
    vertices, faces = torch.as_tensor(vertices), torch.as_tensor(faces)
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertices must be (V,3), got {tuple(vertices.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"faces must be (F,3) int32, got {tuple(faces.shape)} {faces.dtype}")
    return vertices.to(torch.float64).contiguous().to(dev), faces.contiguous().to(dev)


def _views(keys, poses, cams, rays, ray_index):
    """poses, cams, the ray maps and the host ray_index of the views of a key buffer, checked and on its device"""
    from .mvs import camera_rays

    S, H, W = keys.shape
    dev = keys.device
    poses, cams = f64(poses, (S, 3, 4), "poses").to(dev), f64(cams, (S, 4), "cams").to(dev)
    if rays is None:
        rays, ray_index = camera_rays(cams, H, W, dev)
    rays = torch.as_tensor(rays)
    if rays.dim() != 4 or rays.shape[0] < 1:
        raise ValueError(f"rays must be (NR,H,W,2) with NR >= 1, got {tuple(rays.shape)}")
    rays = f64(rays, (rays.shape[0], H, W, 2), "rays")
    if rays.numel() > 0:
        require_gpu(rays)
    if ray_index is None:
        raise ValueError("rays without ray_index")
    ridx = host_i32(ray_index)
    if ridx.numel() != S:
        raise ValueError(f"ray_index must have {S} entries, got {ridx.numel()}")
    if int(ridx.min()) < 0 or int(ridx.max()) >= rays.shape[0]:
        raise ValueError(f"ray_index names a ray map outside [0, {rays.shape[0]})")
    return poses, cams, rays, ridx


def rasterize(keys, vertices, faces, poses, cams, near=1e-6, face_base=0, rays=None, ray_index=None):
    """Draws the faces (F,3) int32 of the vertices (V,3) onto the current contents of `keys` (new_keys) as the views
    poses (S,3,4) [R|t] camera from world, cams (S,4) f, cx, cy, k see them, and returns `keys`.  Face row r is drawn with the
    index face_base + r, so a mesh may be drawn in parts (or several meshes into one buffer) and resolved against the
    concatenated faces.  A face with a vertex at depth <= near is dropped whole; rendering is two-sided.  rays, ray_index:
    the ray maps (NR,H,W,2) and which of them each view uses (default: mvs.camera_rays(cams))."""
    keys = _keys(keys)
    S, H, W = keys.shape
    vertices, faces = _mesh(vertices, faces, keys.device)
    if not float(near) > 0.0:
        raise ValueError(f"near must be > 0, got {near}")
    face_base = int(face_base)
    if face_base < 0 or face_base + faces.shape[0] > Z.MAX_FACES:
        raise ValueError(f"face_base must be >= 0 and face_base + F <= {Z.MAX_FACES}, got {face_base} + {faces.shape[0]}")
    poses, cams, rays, ridx = _views(keys, poses, cams, rays, ray_index)
    check(_L.vggz_raster(vertices, vertices.shape[0], faces, faces.shape[0], face_base, poses, cams, rays, ridx, rays.shape[0],
                         S, H, W, float(near), keys, stream_ptr()), "vggz_raster")
    return keys


def resolve(keys, vertices, faces, poses, cams, normals=None, rgb=None, return_weights=False, rays=None, ray_index=None):
    """The maps of a key buffer drawn from (all of) `faces` -> Rendered(depth (S,H,W) float32, 0 = none; face (S,H,W) int32,
    -1 = none; normal, rgb (S,H,W,3) float32 -- the vertex attributes `normals`, `rgb` (V,3) float32 interpolated with
    perspective-correct weights, the normal renormalised -- or None without the attribute; weights (S,H,W,3) float64, the
    weights of the face's three vertices, or None).  `cams` only chooses the default ray maps."""
    keys = _keys(keys)
    S, H, W = keys.shape
    dev = keys.device
    vertices, faces = _mesh(vertices, faces, dev)
    V = vertices.shape[0]
    attributes = []
    for name, t in (("normals", normals), ("rgb", rgb)):
        if t is not None:
            t = torch.as_tensor(t)
            if tuple(t.shape) != (V, 3) or t.dtype != torch.float32:
                raise ValueError(f"{name} must be ({V},3) float32, got {tuple(t.shape)} {t.dtype}")
            t = t.contiguous().to(dev)
        attributes.append(t)
    normals, rgb = attributes
    poses, cams, rays, ridx = _views(keys, poses, cams, rays, ray_index)
    depth = torch.empty(S, H, W, dtype=torch.float32, device=dev)
    face = torch.empty(S, H, W, dtype=torch.int32, device=dev)
    weights = torch.empty(S, H, W, 3, dtype=torch.float64, device=dev) if return_weights else None
    # (an attribute of an empty mesh has no address: the entry would take it for absent, so its map is zeroed here)
    new = torch.zeros if V == 0 else torch.empty
    out_normal = new(S, H, W, 3, dtype=torch.float32, device=dev) if normals is not None else None
    out_rgb = new(S, H, W, 3, dtype=torch.float32, device=dev) if rgb is not None else None
    check(_L.vggz_resolve(keys, vertices, V, faces, faces.shape[0], normals, rgb, poses, rays, ridx, rays.shape[0], S, H, W,
                          depth, face, weights, out_normal, out_rgb, stream_ptr()), "vggz_resolve")
    return Rendered(depth, face, out_normal, out_rgb, weights)


def render_mesh(mesh_or_vertices, faces=None, *, poses, cams, height, width, normals=True, colors=True, near=1e-6,
                return_weights=False, rays=None, ray_index=None):
    """A mesh rendered into S views of height x width pixels -> Rendered.  mesh_or_vertices: a meshing.Mesh (its normals and
    colours are rendered unless normals / colors is False) or the vertices (V,3), then with `faces` (F,3) int32 and normals /
    colors the attributes (V,3) float32 themselves, or None / False / True for none."""
    if faces is None:
        mesh = mesh_or_vertices
        vertices, faces = mesh.vertices, mesh.faces
        normals = None if normals is None or normals is False else (mesh.normals if normals is True else normals)
        colors = None if colors is None or colors is False else (mesh.rgb if colors is True else colors)
    else:
        vertices = mesh_or_vertices
        normals = None if isinstance(normals, bool) else normals
        colors = None if isinstance(colors, bool) else colors
    vertices = torch.as_tensor(vertices)
    require_gpu(vertices)
    poses = torch.as_tensor(poses)
    if poses.dim() != 3:
        raise ValueError(f"poses must be (S,3,4), got {tuple(poses.shape)}")
    keys = new_keys(poses.shape[0], height, width, vertices.device)
    if rays is None:
        from .mvs import camera_rays

        rays, ray_index = camera_rays(f64(cams, (poses.shape[0], 4), "cams"), int(height), int(width), vertices.device)
    rasterize(keys, vertices, faces, poses, cams, near, 0, rays, ray_index)
    return resolve(keys, vertices, faces, poses, cams, normals, colors, return_weights, rays, ray_index)


def visible_points(points, depth, poses, cams, rel_tol=0.01):
    """points (P,3), depth (S,H,W) float32 (0 = none; a rendered depth, or any depth map) -> (S,P) bool device tensor: the
    point lies in front of camera s, its nearest pixel is in the frame and has a depth z_r, and the point's own depth is
    <= z_r (1 + rel_tol): nothing of the surface hides it."""
    from ._dense_args import maps, views

    depth = maps(depth, "depth")
    S, H, W = depth.shape
    if S < 1:
        raise ValueError("no view")
    if not float(rel_tol) >= 0.0:
        raise ValueError(f"rel_tol must be >= 0, got {rel_tol}")
    points = torch.as_tensor(points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (P,3), got {tuple(points.shape)}")
    points = points.to(torch.float64).contiguous().to(depth.device)
    poses, cams = views(depth, poses, cams)
    out = torch.zeros(S, points.shape[0], dtype=torch.uint8, device=depth.device)
    check(_L.vggz_point_visibility(points, points.shape[0], depth, poses, cams, S, H, W, float(rel_tol), out, stream_ptr()),
          "vggz_point_visibility")
    return out.bool()


def render_reconstruction(reconstruction, mesh, **options):
    """A mesh in the gauge of a reconstruction rendered into every registered image -> (depth_dict, normal_dict, rgb_dict,
    face_dict) by image name: (H,W) float32, (H,W,3) float32, (H,W,3) float32 and (H,W) int32 device tensors.  Views, poses
    and cameras are taken as meshing.mesh_reconstruction takes them (the registered images in id order); every camera must
    have the same size.  `options` are render_mesh's (near, rays, ray_index)."""
    import numpy as np

    from . import dense_depth as DD

    ids = sorted(int(i) for i in reconstruction.reg_image_ids())
    if not ids:
        raise ValueError("nothing to render into: no registered image")
    sizes = {(int(c.height), int(c.width)) for c in (reconstruction.cameras[reconstruction.images[i].camera_id] for i in ids)}
    if len(sizes) != 1:
        raise ValueError(f"the cameras of the registered images differ in size: {sorted(sizes)}")
    H, W = next(iter(sizes))
    pose, cam = DD._camera_rows(reconstruction, ids)
    out = render_mesh(mesh, poses=torch.from_numpy(np.ascontiguousarray(pose)), cams=torch.from_numpy(np.ascontiguousarray(cam)),
                      height=H, width=W, **options)
    names = [reconstruction.images[i].name for i in ids]
    return tuple(None if t is None else {n: t[r] for r, n in enumerate(names)} for t in (out.depth, out.normal, out.rgb, out.face))
