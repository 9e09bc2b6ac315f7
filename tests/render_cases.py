"""Yardstick of the rasteriser tests: a NumPy restatement of vggz_raster, vggz_resolve and vggz_point_visibility from the
text of vggsfm_amd/csrc/raster/vggsfm_amd_raster.h, the cases and their cached references.  A helper, not a test.

Everything is float64 with the header's operation order.  The restatement tests EVERY pixel of a view against every face:
it has no candidate box, which is what checks the kernel's.  (face_box restates the box on its own, for the host test that
every covered pixel lies inside it.)  The cameras are the three of tests/mvs_cases.py's scene, looking at (0, 0, 4)."""
import functools

import numpy as np

from tests import meshing_cases as MC
from tests import mvs_cases as M

EMPTY = np.uint64(2 ** 64 - 1)
SOLO_PIXELS = 64                                                 # VGGZ_SOLO_PIXELS
CHUNK = 512                                                      # faces per (faces x pixels) block of the restatement


# ------------------------------------------------------------------------------------------------------- the rule
def face_setup(vertices, faces, pose, near=None):
    """Per face of one view -> dict: valid (rows in range and distinct, every Xc[2] > near, A > 0 or A < 0), rows_ok, a, b,
    iz (F,3), per edge e (0: 1 -> 2, 1: 2 -> 0, 2: 0 -> 1) ap, bp, da, db, sg (F,3).  near None: no depth test (resolve)."""
    V, F = len(vertices), len(faces)
    f = faces.astype(np.int64).reshape(F, 3)
    rows_ok = ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    P = vertices[np.where(rows_ok[:, None], f, 0)] if V > 0 else np.zeros((F, 3, 3))
    with np.errstate(all="ignore"):
        Xc = [((pose[i, 0] * P[..., 0] + pose[i, 1] * P[..., 1]) + pose[i, 2] * P[..., 2]) + pose[i, 3] for i in range(3)]
        iz = 1.0 / Xc[2]
        a, b = Xc[0] * iz, Xc[1] * iz
        front = np.ones(F, bool) if near is None else (Xc[2] > near).all(1)
        rev = np.stack([f[:, 1] > f[:, 2], f[:, 2] > f[:, 0], f[:, 0] > f[:, 1]], 1)
        u, v = np.array([1, 2, 0]), np.array([2, 0, 1])
        ap, bp = np.where(rev, a[:, v], a[:, u]), np.where(rev, b[:, v], b[:, u])
        da, db = np.where(rev, a[:, u], a[:, v]) - ap, np.where(rev, b[:, u], b[:, v]) - bp
        A = np.where(rev[:, 2], -1.0, 1.0) * (da[:, 2] * (b[:, 2] - bp[:, 2]) - db[:, 2] * (a[:, 2] - ap[:, 2]))
        neg = A < 0.0
        valid = rows_ok & front & ((A > 0.0) | (A < 0.0))
    sg = np.where(rev != neg[:, None], -1.0, 1.0)
    return dict(valid=valid, rows_ok=rows_ok, a=a, b=b, iz=iz, ap=ap, bp=bp, da=da, db=db, sg=sg, A=A)


def edge_weights(st, sel, ra, rb):
    """w_e (3, n, P) of the faces `sel` (indices or a slice) at the rays (ra, rb) (P,): every pixel against every face"""
    return [st["sg"][sel, e, None] * (st["da"][sel, e, None] * (rb[None] - st["bp"][sel, e, None]) -
                                      st["db"][sel, e, None] * (ra[None] - st["ap"][sel, e, None])) for e in range(3)]


def _shade(st, sel, w):
    """lambda_j, q of edge weights w (each aligned with the faces `sel` on axis 0)"""
    iz = st["iz"][sel]
    iz = [iz[:, j, None] if w[0].ndim == 2 else iz[:, j] for j in range(3)]
    with np.errstate(all="ignore"):
        total = (w[0] + w[1]) + w[2]
        lam = [w[j] / total for j in range(3)]
        q = (lam[0] * iz[0] + lam[1] * iz[1]) + lam[2] * iz[2]
    return lam, q, total, iz


def raster(keys, vertices, faces, face_base, poses, cams, rays, ray_index, near, detail=False):
    """vggz_raster on a copy of keys (S,H,W) uint64 -> keys (and, detail=True, per view the (F, H W) bool mask of the
    pixels each face covers and the smallest nonzero |w_j| over the valid faces and all pixels)."""
    S, H, W = keys.shape
    out = keys.copy().reshape(S, H * W)
    F = len(faces)
    covered_all, margin = [], np.inf
    for s in range(S):
        st = face_setup(vertices, faces, poses[s], near)
        ra, rb = rays[ray_index[s]].reshape(-1, 2).T
        cov_view = np.zeros((F, H * W), bool)
        for lo in range(0, F, CHUNK):
            sel = slice(lo, min(F, lo + CHUNK))
            w = edge_weights(st, sel, ra, rb)
            lam, q, total, _ = _shade(st, sel, w)
            with np.errstate(all="ignore"):
                covered = (w[0] >= 0.0) & (w[1] >= 0.0) & (w[2] >= 0.0) & (total > 0.0) & st["valid"][sel, None]
                zf = (1.0 / q).astype(np.float32)
                ok = covered & (zf > 0) & np.isfinite(zf)
            g = (np.arange(lo, lo + covered.shape[0], dtype=np.uint64) + np.uint64(face_base))[:, None]
            key = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | g
            key = np.where(ok, key, EMPTY)
            if key.shape[0]:
                out[s] = np.minimum(out[s], key.min(0))
            if detail:
                cov_view[sel] = ok
                for j in range(3):
                    aw = np.abs(w[j][st["valid"][sel]])
                    aw = aw[aw > 0.0]
                    margin = min(margin, float(aw.min(initial=np.inf)))
        covered_all.append(cov_view)
    out = out.reshape(S, H, W)
    return (out, covered_all, margin) if detail else out


def resolve(keys, vertices, faces, normals, rgb, poses, rays, ray_index):
    """vggz_resolve -> dict depth (S,H,W) f4, face (S,H,W) i4, weights (S,H,W,3) f8, normal, rgb (S,H,W,3) f4 or None"""
    S, H, W = keys.shape
    F, V = len(faces), len(vertices)
    depth, face = np.zeros((S, H * W), np.float32), np.full((S, H * W), -1, np.int32)
    weights = np.zeros((S, H * W, 3))
    out_n = None if normals is None else np.zeros((S, H * W, 3), np.float32)
    out_c = None if rgb is None else np.zeros((S, H * W, 3), np.float32)
    for s in range(S):
        k = keys[s].reshape(-1)
        g = (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
        st = face_setup(vertices, faces, poses[s], None)
        hit = (k != EMPTY) & (g < F)
        hit[hit] = st["rows_ok"][g[hit]]
        px = np.nonzero(hit)[0]
        if len(px) == 0:
            continue
        gs = g[px]
        ra, rb = rays[ray_index[s]].reshape(-1, 2)[px].T
        w = [st["sg"][gs, e] * (st["da"][gs, e] * (rb - st["bp"][gs, e]) - st["db"][gs, e] * (ra - st["ap"][gs, e]))
             for e in range(3)]
        lam, q, _, iz = _shade(st, gs, w)
        with np.errstate(all="ignore"):
            om = [(lam[j] * iz[j]) / q for j in range(3)]
        depth[s, px] = (k[px] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        face[s, px] = gs
        weights[s, px] = np.stack(om, -1)
        rows = faces.astype(np.int64)[gs]
        for attr, out, unit in ((normals, out_n, True), (rgb, out_c, False)):
            if attr is None:
                continue
            N = attr.astype(np.float64)[rows]                                  # (n, 3 vertices, 3 components)
            with np.errstate(all="ignore"):
                G = [(om[0] * N[:, 0, c] + om[1] * N[:, 1, c]) + om[2] * N[:, 2, c] for c in range(3)]
                if unit:
                    ln = np.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
                    G = [np.where(ln > 0.0, G[c] / ln, 0.0) for c in range(3)]
            out[s, px] = np.stack(G, -1).astype(np.float32)
    sh = lambda t: None if t is None else t.reshape(S, H, W, 3)
    return dict(depth=depth.reshape(S, H, W), face=face.reshape(S, H, W), weights=sh(weights), normal=sh(out_n), rgb=sh(out_c))


def render(vertices, faces, normals, rgb, poses, cams, rays, ray_index, H, W, near=1e-6):
    """new keys, raster, resolve -> the dict of resolve with `keys` added"""
    keys = np.full((len(poses), H, W), EMPTY, np.uint64)
    keys = raster(keys, vertices, faces, 0, poses, cams, rays, ray_index, near)
    out = resolve(keys, vertices, faces, normals, rgb, poses, rays, ray_index)
    out["keys"] = keys
    return out


def face_box(vertices, faces, pose, cam, near, H, W):
    """The header's candidate box per face of one view -> has (F,) bool, x0, x1, y0, y1 (F,) int (clamped to the frame)"""
    st = face_setup(vertices, faces, pose, near)
    a, b = st["a"], st["b"]
    with np.errstate(all="ignore"):
        d = 1.0 + cam[3] * (a * a + b * b)
        x, y = cam[0] * (a * d) + cam[1], cam[0] * (b * d) + cam[2]
        r = np.sqrt((a * a + b * b).max(1))
        nx = np.array([1, 2, 0])
        L2 = ((a[:, nx] - a) ** 2 + (b[:, nx] - b) ** 2).max(1)
        m = 1.0 + 0.75 * cam[0] * abs(cam[3]) * r * L2
        bx0, bx1 = np.floor(x.min(1) - m), np.ceil(x.max(1) + m)
        by0, by1 = np.floor(y.min(1) - m), np.ceil(y.max(1) + m)
        has = st["valid"] & np.isfinite(x).all(1) & np.isfinite(y).all(1) & (m >= 1.0) & (bx1 >= 0) & (bx0 <= W - 1) & \
            (by1 >= 0) & (by0 <= H - 1)
    cl = lambda v, hi: np.where(has, np.clip(np.nan_to_num(v, nan=0.0, posinf=1e9, neginf=-1e9), 0, hi), 0).astype(np.int64)
    return has, cl(bx0, W - 1), cl(bx1, W - 1), cl(by0, H - 1), cl(by1, H - 1)


def point_visibility(points, depth, poses, cams, rel_tol, detail=False):
    """vggz_point_visibility -> (S,P) uint8 (and, detail=True, the margins: round (distance of x + 0.5, y + 0.5 from an
    integer over the points in front), tol (|Xc[2] - z_r (1 + rel_tol)| over the points that reach that test), front)"""
    S, H, W = depth.shape
    out = np.zeros((S, len(points)), np.uint8)
    mg = dict(round=np.inf, tol=np.inf, front=np.inf)
    for s in range(S):
        x, y, zc = M.transfer_project(poses[s], cams[s], points[:, 0], points[:, 1], points[:, 2])
        with np.errstate(invalid="ignore"):
            front = zc > 0.0
            xi, yi = np.floor(x + 0.5), np.floor(y + 0.5)
            go = front & M.inside_image(xi, yi, H, W)
        xq, yq = np.where(go, xi, 0).astype(np.int64), np.where(go, yi, 0).astype(np.int64)
        zr = depth[s].astype(np.float64)[yq, xq] if H * W > 0 else np.zeros(len(points))
        go = go & (zr > 0.0)
        lim = zr * (1.0 + rel_tol)
        with np.errstate(invalid="ignore"):
            out[s] = go & (zc <= lim)
        mg["front"] = min(mg["front"], float(np.abs(zc).min(initial=np.inf)))
        if front.any():
            fr = np.stack([x[front] + 0.5, y[front] + 0.5])
            mg["round"] = min(mg["round"], float(np.abs(fr - np.round(fr)).min()))
        mg["tol"] = min(mg["tol"], float(np.abs(zc - lim)[go].min(initial=np.inf)))
    return (out, mg) if detail else out


# ------------------------------------------------------------------------------------------------------- cameras
@functools.lru_cache(maxsize=None)
def cameras():
    """name -> dict poses (3,3,4), cams (3,4), rays (NR,H,W,2), ray_index (3,), H, W: the three cameras of mvs_cases.scene"""
    def one(H, W, k):
        sc = M.scene(H=H, W=W, k=k)
        return dict(poses=sc["poses"], cams=sc["cams"], rays=sc["rays"], ray_index=sc["ray_index"], H=H, W=W)
    out = {"k0": one(24, 32, 0.0), "k08": one(24, 32, 0.08), "km10": one(24, 32, -0.1), "odd_k08": one(21, 35, 0.08),
           "odd_km10": one(21, 35, -0.1)}
    # two distinct camera rows among the three views: the middle view has a camera (and a ray map) of its own
    a = out["k08"]
    other = np.array([36.0, 15.1, 11.9, 0.0])
    cams = a["cams"].copy()
    cams[1] = other
    out["two_cams"] = dict(poses=a["poses"], cams=cams, rays=np.stack([a["rays"][0], M.pixel_rays(other, 24, 32)]),
                           ray_index=np.array([0, 1, 0], np.int32), H=24, W=32)
    # the middle camera at the origin looking along +z: pixel x = f X / Z + cx, for the faces with boxes of a chosen size
    b = out["k0"]
    poses = b["poses"].copy()
    poses[1] = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    out["straight"] = dict(b, poses=poses)
    for c in out.values():
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------- meshes
PLANE = (2.0, 0.3, 0.1)                                         # z = 2 + 0.3 x + 0.1 y
SPHERE_SCALE, SPHERE_AT = 0.15, np.array([0.05, -0.03, 3.0])    # the 13 x 11 x 10 sphere volume's mesh, scaled and placed


def _attributes(vertices, seed):
    """unit normals and colours (V,3) float32 per vertex: smooth in the position, so that interpolation has something to do"""
    g = np.random.default_rng(seed)
    n = np.stack([0.3 * np.sin(vertices[:, 0] * 2.0), 0.3 * np.cos(vertices[:, 1] * 3.0), -np.ones(len(vertices))], -1)
    n = n + 0.05 * g.standard_normal(n.shape)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    c = np.stack([0.5 + 0.2 * vertices[:, 0], 0.5 - 0.3 * vertices[:, 1], 0.1 * vertices[:, 2]], -1)
    return n.astype(np.float32), c.astype(np.float32)


def plane_mesh(seed=1):
    """a jittered 9 x 9 grid on the slanted plane, 128 faces, the vertex rows shuffled"""
    g = np.random.default_rng(seed)
    j, i = np.mgrid[0:9, 0:9]
    x = -1.6 + 0.4 * i + g.uniform(-0.1, 0.1, i.shape) * ((i > 0) & (i < 8))
    y = -1.2 + 0.3 * j + g.uniform(-0.075, 0.075, j.shape) * ((j > 0) & (j < 8))
    v = np.stack([x, y, PLANE[0] + PLANE[1] * x + PLANE[2] * y], -1).reshape(81, 3)
    n = lambda jj, ii: jj * 9 + ii
    faces = []
    for jj in range(8):
        for ii in range(8):
            q = [n(jj, ii), n(jj, ii + 1), n(jj + 1, ii + 1), n(jj + 1, ii)]
            faces += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]] if (ii + jj) % 2 else [[q[0], q[1], q[3]], [q[1], q[2], q[3]]]
    perm = g.permutation(81)                                                 # new row of old vertex i: perm[i]
    out = np.empty_like(v)
    out[perm] = v
    return out, perm[np.array(faces)].astype(np.int32)


def sphere_mesh():
    ref = MC.volume_reference("sphere")
    v = (ref["vertices"] - MC.SPHERE_CENTRE) * SPHERE_SCALE + SPHERE_AT
    return np.ascontiguousarray(v), ref["faces"].copy(), ref["normals"].copy(), ref["rgb"].copy()


def _quad(x0, x1, y0, y1, z, dzdx=0.0):
    v = np.array([[x0, y0, z + dzdx * x0], [x1, y0, z + dzdx * x1], [x1, y1, z + dzdx * x1], [x0, y1, z + dzdx * x0]])
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def _join(parts):
    """meshes (vertices, faces) concatenated"""
    vs, fs, base = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def box_sizes_mesh(cam):
    """70 faces for the camera at the origin looking along +z (view 1 of cameras()["straight"]): triangles whose candidate
    boxes there hold 1, 63, 64, 65 and 690 pixels, interleaved, each at a depth of its own.  A triangle with pixel bounds
    [i + 0.5, j + 0.5] has the box i - 1 .. j + 2 (k = 0: the margin is exactly 1)."""
    f, cx, cy, _ = cam
    kinds = [None, (5, 3), (4, 4), (9, 1), (26, 19)]                          # (j - i) in x and y: 9x7, 8x8, 13x5, 30x23
    parts = []
    for n in range(70):
        kind = kinds[n % 5]
        z = 3.0 + 0.013 * n
        if kind is None:                                                     # just outside the corner: the box is pixel (0, 0)
            px = np.array([[-1.3171, -1.4093], [-1.1037, -1.3529], [-1.2213, -1.1561]]) - np.array([0.0113, 0.0097]) * (n // 5)
        else:
            ox, oy = 1 + (n // 5) % (29 - kind[0] - 2 + 1), 1 + (n // 5) % (21 - kind[1] - 2 + 1)
            x0, x1, y0, y1 = ox + 0.5, ox + kind[0] + 0.5, oy + 0.5, oy + kind[1] + 0.5
            al, be = 0.3713 + 0.00291 * n, 0.4127 - 0.00173 * n              # (generic: no edge runs through a pixel centre)
            px = np.array([[x0, y0], [x1, y0 + al * (y1 - y0)], [x0 + be * (x1 - x0), y1]])
        v = np.stack([(px[:, 0] - cx) / f * z, (px[:, 1] - cy) / f * z, np.full(3, z)], -1)
        parts.append((v, np.array([[0, 1, 2]], np.int32)))
    return _join(parts)


def skippable_mesh():
    """one good face and every face the rule skips; near = 2.0 for this case"""
    nan = float("nan")
    v = np.array([[-0.4, -0.3, 3.1], [0.5, -0.2, 3.3], [0.1, 0.4, 3.2],          # 0 1 2: the good face
                  [-0.4, -0.3, -3.1], [0.5, -0.2, -3.3], [0.1, 0.4, -3.2],       # 3 4 5: behind the cameras
                  [-0.3, 0.2, 1.5], [0.3, 0.25, 3.0], [0.0, -0.3, 2.9],          # 6 7 8: straddles near = 2
                  [-0.2, -0.1, 2.8], [-0.2, -0.1, 2.8], [0.3, 0.1, 2.7],         # 9 10 11: rows 9 and 10 coincide: zero area
                  [0.1, nan, 2.5],                                                # 12: a NaN vertex
                  [7.0, 5.0, 3.0], [7.5, 5.0, 3.0], [7.0, 5.6, 3.1]])             # 13 14 15: wholly outside every frame
    f = np.array([[3, 4, 5], [6, 7, 8], [0, 1, 1], [9, 10, 11], [0, 1, 16], [0, -1, 2], [0, 12, 2], [13, 14, 15], [0, 1, 2],
                  [2, 2, 2], [1, 0, 2 ** 31 - 1]], np.int32)
    return v, f


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict vertices, faces, normals, rgb, near and the camera dict's entries"""
    cam = cameras()

    def mk(mesh, c, near=1e-6, seed=2, attrs=None):
        v, f = mesh
        n, col = _attributes(v, seed) if attrs is None else attrs
        case = dict(vertices=np.ascontiguousarray(v, np.float64), faces=np.ascontiguousarray(f, np.int32), normals=n, rgb=col,
                    near=near)
        case.update(cam[c])
        for t in case.values():
            if isinstance(t, np.ndarray):
                t.setflags(write=False)
        return case

    sv, sf, sn, sc = sphere_mesh()
    quads = _join([_quad(-1.43, 1.37, -1.13, 1.09, 3.5), _quad(-0.31, 0.29, -0.21, 0.23, 2.5)])
    tri = (np.array([[-0.33, -0.21, 2.9], [0.41, -0.12, 3.1], [0.07, 0.37, 3.0]]), np.array([[0, 1, 2], [0, 1, 2]], np.int32))
    fill = _quad(-2.03, 1.71, -1.31, 1.19, 3.0, 0.1)
    out = {
        "plane_k0": mk(plane_mesh(), "k0"), "plane_k08": mk(plane_mesh(), "k08"), "plane_km10": mk(plane_mesh(), "km10"),
        "plane_21x35": mk(plane_mesh(), "odd_k08"), "plane_two_cams": mk(plane_mesh(), "two_cams"),
        "sphere_k08": mk((sv, sf), "k08", attrs=(sn, sc)), "sphere_21x35": mk((sv, sf), "odd_km10", attrs=(sn, sc)),
        "occluding_quads": mk(quads, "k08"), "same_face_twice": mk(tri, "k08"),
        "fill_k08": mk(fill, "k08"), "fill_km10": mk(fill, "km10"), "fill_21x35": mk(fill, "odd_km10"),
        "box_sizes": mk(box_sizes_mesh(cam["straight"]["cams"][1]), "straight"),
        "skippable": mk(skippable_mesh(), "k08", near=2.0), "skippable_21x35": mk(skippable_mesh(), "odd_k08", near=2.0),
        "one_face": mk((tri[0], tri[1][:1]), "k0"), "no_face": mk((tri[0], tri[1][:0]), "k0"),
    }
    return out


TIE_FREE = tuple(n for n in ("plane_k0", "plane_k08", "plane_km10", "plane_21x35", "plane_two_cams", "sphere_k08", "sphere_21x35",
                             "occluding_quads", "fill_k08", "fill_km10", "fill_21x35", "box_sizes", "skippable", "skippable_21x35",
                             "one_face", "no_face"))


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's render of a case -- computed once, never modified; with `covered` (per view (F, H W) bool) and
    `margin` (the smallest nonzero |w_j|)"""
    c = cases()[name]
    S, H, W = len(c["poses"]), c["H"], c["W"]
    keys = np.full((S, H, W), EMPTY, np.uint64)
    keys, covered, margin = raster(keys, c["vertices"], c["faces"], 0, c["poses"], c["cams"], c["rays"], c["ray_index"],
                                   c["near"], detail=True)
    out = resolve(keys, c["vertices"], c["faces"], c["normals"], c["rgb"], c["poses"], c["rays"], c["ray_index"])
    out.update(keys=keys, covered=covered, margin=margin)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------- truth
def pixel_world_rays(pose, rays):
    """camera centre (3,) and world directions (H,W,3) of a ray map, scaled so that camera-frame z = the parameter"""
    R, t = pose[:, :3], pose[:, 3]
    return -R.T @ t, np.concatenate([rays, np.ones(rays.shape[:2] + (1,))], -1) @ R


def plane_depth(pose, rays):
    """camera-frame z (H,W) of the slanted plane z = 2 + 0.3 x + 0.1 y along every ray"""
    c, d = pixel_world_rays(pose, rays)
    nrm = np.array([-PLANE[1], -PLANE[2], 1.0])
    return (PLANE[0] - nrm @ c) / (d @ nrm)


# ------------------------------------------------------------------------------------------------------- visibility
@functools.lru_cache(maxsize=None)
def visibility_case():
    """200 points before, on and behind the sphere seen by the k08 cameras, against the restatement's render of it"""
    c, ref = cases()["sphere_k08"], reference("sphere_k08")
    g = np.random.default_rng(9)
    d = g.standard_normal((200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    on = SPHERE_AT + d * (MC.SPHERE_RADIUS * SPHERE_SCALE)
    # (the middle camera stands at the origin: a point scaled towards it keeps its pixel there)
    pts = on * np.concatenate([np.full(70, 0.7), np.full(60, 1.0), np.full(70, 1.4)])[:, None]
    pts[:10] += np.array([0.0, 0.0, -5.0])                                   # behind the cameras
    pts[10:20] += np.array([3.0, 0.0, 0.0])                                  # outside the frames
    pts[20] = np.nan
    out = dict(points=pts, depth=ref["depth"], poses=c["poses"], cams=c["cams"], rel_tol=0.01)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
