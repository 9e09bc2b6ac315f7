"""Yardstick of the meshing tests: a NumPy restatement of vggv_integrate, vggv_mesh_count and vggv_mesh_emit from the text of
vggsfm_amd/csrc/tsdf/vggsfm_amd_tsdf.h, the 16-case table DERIVED from the header's geometric rule (never copied from the
kernel), the cases and their cached references.  A helper, not a test.

Everything is float64 from the float32 inputs, vectorised over the nodes of the grid, with the header's operation order.  The
integration scenes are the analytic ones of tests/mvs_cases.py (a slanted, textured plane seen from a line of cameras) with
their true depths rounded to float32; the extraction fields (spheres, a plane) are written directly as volumes."""
import functools
import itertools

import numpy as np

from tests import fusion_cases as FC
from tests import mvs_cases as M

GROUP = 256                                                     # VGGV_GROUP: nodes per group of the two-level count
EDGE_DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMS = tuple(itertools.permutations(range(3)))                 # lexicographic
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def perm_sign(seq):
    """sign of a sequence of distinct numbers read as a permutation (parity of its inversions)"""
    inv = sum(1 for i in range(len(seq)) for j in range(i + 1, len(seq)) if seq[i] > seq[j])
    return -1 if inv & 1 else 1


def tet_corners(t):
    """the four corners of tetrahedron t of a cell as offsets (dx, dy, dz): p0 = the cell's node, p_{m+1} = p_m + e_pi(m)"""
    p = [0, 0, 0]
    out = [tuple(p)]
    for axis in PERMS[t]:
        p[axis] += 1
        out.append(tuple(p))
    return out


def derive_case_table():
    """(2, 16, 7) int32 from the header's rule: [0] for sigma = +1, [1] for sigma = -1; bit c of the pattern set = corner c
    inside; a row is the number of triangles and then per triangle its three vertices as indices into TET_EDGES, -1 unused."""
    table = np.full((2, 16, 7), -1, np.int32)
    eid = {e: i for i, e in enumerate(TET_EDGES)}
    v = lambda x, y: eid[(min(x, y), max(x, y))]
    for si, sigma in enumerate((1, -1)):
        for pattern in range(16):
            inside = [c for c in range(4) if pattern >> c & 1]
            outside = [c for c in range(4) if not pattern >> c & 1]
            tris = []
            if len(inside) in (1, 3):
                lone, rest, side = (inside[0], outside, 1) if len(inside) == 1 else (outside[0], inside, -1)
                tri = [v(lone, o) for o in rest]
                if perm_sign([lone] + rest) * sigma * side < 0:
                    tri[1], tri[2] = tri[2], tri[1]
                tris = [tri]
            elif len(inside) == 2:
                (a, b), (c, d) = inside, outside
                q = [v(a, c), v(a, d), v(b, d), v(b, c)]
                if perm_sign([a, b, c, d]) * sigma < 0:
                    q.reverse()
                tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
            table[si, pattern, 0] = len(tris)
            for r, tri in enumerate(tris):
                table[si, pattern, 1 + 3 * r:4 + 3 * r] = tri
    return table


# ------------------------------------------------------------------------------------------------------- the grid
def node_positions(origin, voxel, dims):
    """X[c] (nz, ny, nx) of every node: origin[c] + voxel * index"""
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return [origin[0] + voxel * i.astype(np.float64), origin[1] + voxel * j.astype(np.float64),
            origin[2] + voxel * k.astype(np.float64)]


def empty_volume(dims, color=True):
    N = dims[0] * dims[1] * dims[2]
    return np.zeros(N), np.zeros(N), (np.zeros((N, 3)) if color else None)


# ------------------------------------------------------------------------------------------------------- entry 1
def integrate(depth, weights, frames, poses, cams, origin, voxel, dims, trunc, tsdf_sum, weight_sum, rgb_sum):
    """vggv_integrate on copies of the volumes -> (tsdf_sum, weight_sum, rgb_sum, margins).  margins: front (|Xc[2]|), round
    (distance of x + 0.5, y + 0.5 from an integer), trunc (|sdf + trunc|) over the samples that reach each test."""
    S, H, W = depth.shape
    nx, ny, nz = dims
    X = [c.reshape(-1) for c in node_positions(origin, voxel, dims)]
    tsdf, wsum = tsdf_sum.copy(), weight_sum.copy()
    rgb = None if rgb_sum is None else rgb_sum.copy()
    mg = dict(front=np.inf, round=np.inf, trunc=np.inf)
    for s in range(S):
        x, y, zc = M.transfer_project(poses[s], cams[s], X[0], X[1], X[2])
        with np.errstate(invalid="ignore"):
            front = zc > 0.0
            xi, yi = np.floor(x + 0.5), np.floor(y + 0.5)
            go = front & M.inside_image(xi, yi, H, W)
        mg["front"] = min(mg["front"], float(np.abs(zc).min(initial=np.inf)))
        if front.any():
            fr = np.stack([x[front] + 0.5, y[front] + 0.5])
            mg["round"] = min(mg["round"], float(np.abs(fr - np.round(fr)).min()))
        xq, yq = np.where(go, xi, 0).astype(np.int64), np.where(go, yi, 0).astype(np.int64)
        z = depth[s].astype(np.float64)[yq, xq]
        go = go & (z > 0.0)
        w = np.ones(len(z)) if weights is None else weights[s].astype(np.float64)[yq, xq]
        go = go & (w > 0.0)
        sdf = z - zc
        mg["trunc"] = min(mg["trunc"], float(np.abs(sdf + trunc)[go].min(initial=np.inf)))
        with np.errstate(invalid="ignore"):
            go = go & (sdf >= -trunc)
        d = np.minimum(1.0, sdf / trunc)
        tsdf = np.where(go, tsdf + w * d, tsdf)
        wsum = np.where(go, wsum + w, wsum)
        if rgb is not None and frames is not None:
            for c in range(3):
                col = frames[s, c].astype(np.float64)[yq, xq]
                rgb[:, c] = np.where(go, rgb[:, c] + w * col, rgb[:, c])
    return tsdf, wsum, rgb, mg


# ------------------------------------------------------------------------------------------------------- level set
def _shift(a, d, fill):
    """a (nz, ny, nx) read at +d = (dx, dy, dz); `fill` where that node does not exist"""
    dx, dy, dz = d
    out = np.full(a.shape, fill, a.dtype)
    nz, ny, nx = a.shape
    src = a[max(dz, 0):nz + min(dz, 0) or None, max(dy, 0):ny + min(dy, 0) or None, max(dx, 0):nx + min(dx, 0) or None]
    out[max(-dz, 0):nz - max(dz, 0), max(-dy, 0):ny - max(dy, 0), max(-dx, 0):nx - max(dx, 0)] = src
    return out


def _values(tsdf_sum, weight_sum, dims, min_weight):
    nx, ny, nz = dims
    w = weight_sum.reshape(nz, ny, nx)
    with np.errstate(invalid="ignore"):
        valid = w >= min_weight
    with np.errstate(all="ignore"):
        s = tsdf_sum.reshape(nz, ny, nx) / w
    with np.errstate(invalid="ignore"):
        inside = s < 0.0
    return s, valid, inside


def _offset(code, dims):
    return (code & 1) + (code >> 1 & 1) * dims[0] + (code >> 2 & 1) * dims[0] * dims[1]


def _code(d):
    return d[0] + 2 * d[1] + 4 * d[2]


EDGE_OF_CODE = {_code(d): e for e, d in enumerate(EDGE_DIRS)}


def mesh_count(tsdf_sum, weight_sum, dims, min_weight):
    """vggv_mesh_count -> dict: edge_mask (N) uint8, vertex_offset, face_offset (N) int32 (inside the node's group of 256),
    group_counts (G, 2) int32, group_offsets (G, 2) int64, counts (2) int64, and margins: value (smallest |s| at a valid
    node), weight (smallest |weight_sum - min_weight|)."""
    nx, ny, nz = dims
    N = nx * ny * nz
    s, valid, inside = _values(tsdf_sum, weight_sum, dims, min_weight)
    mask = np.zeros((nz, ny, nx), np.uint8)
    for e, d in enumerate(EDGE_DIRS):
        vb, ib = _shift(valid, d, False), _shift(inside, d, False)
        mask |= ((valid & vb & (inside != ib)).astype(np.uint8) << e).astype(np.uint8)
    nv = np.zeros((nz, ny, nx), np.int32)
    for e in range(7):
        nv += mask >> e & 1
    cell = np.zeros((nz, ny, nx), bool)
    cell[:nz - 1, :ny - 1, :nx - 1] = True
    ntri = derive_case_table()[0, :, 0]
    nf = np.zeros((nz, ny, nx), np.int32)
    for t in range(6):
        ok, pattern = cell.copy(), np.zeros((nz, ny, nx), np.int64)
        for c, d in enumerate(tet_corners(t)):
            ok &= _shift(valid, d, False)
            pattern |= _shift(inside, d, False).astype(np.int64) << c
        nf += np.where(ok, ntri[pattern], 0).astype(np.int32)
    G = -(-N // GROUP)
    pad = G * GROUP - N
    out = {"edge_mask": mask.reshape(-1)}
    group_counts = np.zeros((G, 2), np.int32)
    for col, (name, cnt) in enumerate((("vertex_offset", nv), ("face_offset", nf))):
        c = np.concatenate([cnt.reshape(-1), np.zeros(pad, np.int32)]).reshape(G, GROUP).astype(np.int64)
        incl = np.cumsum(c, 1)
        out[name] = (incl - c).reshape(-1)[:N].astype(np.int32)
        group_counts[:, col] = incl[:, -1]
    total = np.cumsum(group_counts.astype(np.int64), 0)
    out["group_counts"] = group_counts
    out["group_offsets"] = (total - group_counts).astype(np.int64)
    out["counts"] = total[-1].astype(np.int64)
    vv = np.abs(s[valid])
    out["margins"] = dict(value=float(vv.min(initial=np.inf)),
                          weight=float(np.abs(weight_sum - min_weight).min(initial=np.inf)))
    return out


def gradients(s, valid, voxel):
    """the header's gradient of s per node -> g (3, nz, ny, nx) and `has`; meaningful at valid nodes only"""
    g, has = [], np.ones(s.shape, bool)
    for axis in range(3):
        d = tuple(1 if a == axis else 0 for a in range(3))
        m = tuple(-c for c in d)
        vp, vm = _shift(valid, d, False), _shift(valid, m, False)
        sp, sm = _shift(s, d, 0.0), _shift(s, m, 0.0)
        with np.errstate(all="ignore"):
            both, plus, minus = (sp - sm) / (2.0 * voxel), (sp - s) / voxel, (s - sm) / voxel
        g.append(np.where(vp & vm, both, np.where(vp, plus, minus)))
        has &= vp | vm
    return np.stack(g), has


def mesh_emit(tsdf_sum, weight_sum, rgb_sum, origin, voxel, dims, min_weight, count):
    """vggv_mesh_emit from the outputs of mesh_count -> dict: vertices (V, 3) float64, normals, rgb (V, 3) float32 (rgb zeros
    without rgb_sum), faces (F, 3) int32, vertex_edge (V, 2) int64 (owner node, edge) and the margin `gradient` (smallest
    |g| over the vertices whose two gradients exist)."""
    nx, ny, nz = dims
    s, valid, inside = _values(tsdf_sum, weight_sum, dims, min_weight)
    X = node_positions(origin, voxel, dims)
    g, has = gradients(s, valid, voxel)
    mask = count["edge_mask"].reshape(nz, ny, nx)
    w = weight_sum.reshape(nz, ny, nx)
    with np.errstate(all="ignore"):
        col = None if rgb_sum is None else [rgb_sum[:, c].reshape(nz, ny, nx) / w for c in range(3)]
    keys, pos, nrm, rgb = [], [], [], []
    m_grad = np.inf
    node = np.arange(nx * ny * nz).reshape(nz, ny, nx)
    for e, d in enumerate(EDGE_DIRS):
        sel = (mask >> e & 1).astype(bool)
        if not sel.any():
            continue
        sa, sb = s[sel], _shift(s, d, 0.0)[sel]
        t = sa / (sa - sb)
        pos.append(np.stack([X[c][sel] + t * (_shift(X[c], d, 0.0)[sel] - X[c][sel]) for c in range(3)], -1))
        gv = [g[c][sel] + t * (_shift(g[c], d, 0.0)[sel] - g[c][sel]) for c in range(3)]
        length = np.sqrt((gv[0] * gv[0] + gv[1] * gv[1]) + gv[2] * gv[2])
        ok = has[sel] & _shift(has, d, False)[sel]
        m_grad = min(m_grad, float(length[ok].min(initial=np.inf)))
        with np.errstate(invalid="ignore"):
            ok = ok & (length > 0.0)
        with np.errstate(all="ignore"):
            nrm.append(np.stack([np.where(ok, gv[c] / length, 0.0).astype(np.float32) for c in range(3)], -1))
        if col is not None:
            rgb.append(np.stack([(col[c][sel] + t * (_shift(col[c], d, 0.0)[sel] - col[c][sel])).astype(np.float32)
                                 for c in range(3)], -1))
        keys.append(np.stack([node[sel], np.full(int(sel.sum()), e)], -1))
    if keys:
        keys = np.concatenate(keys)
        order = np.lexsort((keys[:, 1], keys[:, 0]))
        keys, pos, nrm = keys[order], np.concatenate(pos)[order], np.concatenate(nrm)[order]
        rgb = np.concatenate(rgb)[order] if col is not None else np.zeros((len(keys), 3), np.float32)
    else:
        keys, pos = np.zeros((0, 2), np.int64), np.zeros((0, 3))
        nrm, rgb = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
    assert len(pos) == int(count["counts"][0])

    # faces: the vertex of an edge is the owner's first row plus the set bits below the edge in its mask
    table = derive_case_table()
    first = count["group_offsets"][np.arange(nx * ny * nz) // GROUP, 0] + count["vertex_offset"]
    flat_mask = count["edge_mask"].astype(np.int64)
    below = lambda owner, e: first[owner] + np.array([bin(v).count("1") for v in flat_mask[owner] & ((1 << e) - 1)], np.int64)
    cell = np.zeros((nz, ny, nx), bool)
    cell[:nz - 1, :ny - 1, :nx - 1] = True
    rows = []
    for t in range(6):
        corners = tet_corners(t)
        codes = np.array([_code(c) for c in corners])
        si = 0 if perm_sign(PERMS[t]) > 0 else 1
        ok, pattern = cell.copy(), np.zeros((nz, ny, nx), np.int64)
        for c, d in enumerate(corners):
            ok &= _shift(valid, d, False)
            pattern |= _shift(inside, d, False).astype(np.int64) << c
        for r in range(2):
            sel = ok & (table[si, :, 0][pattern] > r)
            if not sel.any():
                continue
            n0, pat = node[sel], pattern[sel]
            tri = []
            for q in range(3):
                eid = table[si][pat, 1 + 3 * r + q]
                x, y = np.array(TET_EDGES)[eid].T
                owner = n0 + np.array([_offset(int(c), dims) for c in codes])[x]
                edge = np.array([EDGE_OF_CODE.get(int(c), -1) for c in range(8)])[codes[y] ^ codes[x]]
                ids = np.empty(len(n0), np.int64)
                for e in range(7):
                    hit = edge == e
                    if hit.any():
                        assert (flat_mask[owner[hit]] >> e & 1).all()          # a face names vertices that exist
                        ids[hit] = below(owner[hit], e)
                tri.append(ids)
            rows.append(np.stack([n0, np.full(len(n0), t), np.full(len(n0), r)] + tri, -1))
    if rows:
        rows = np.concatenate(rows)
        rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
        faces = rows[:, 3:].astype(np.int32)
    else:
        faces = np.zeros((0, 3), np.int32)
    assert len(faces) == int(count["counts"][1])
    return {"vertices": pos, "normals": nrm, "rgb": rgb, "faces": faces, "vertex_edge": keys, "margins": {"gradient": m_grad}}


def extract(tsdf_sum, weight_sum, rgb_sum, origin, voxel, dims, min_weight):
    """count, then emit -> the two dicts merged (margins merged too)"""
    count = mesh_count(tsdf_sum, weight_sum, dims, min_weight)
    mesh = mesh_emit(tsdf_sum, weight_sum, rgb_sum, origin, voxel, dims, min_weight, count)
    out = dict(count, **mesh)
    out["margins"] = dict(count["margins"], **mesh["margins"])
    return out


# ------------------------------------------------------------------------------------------------------- mesh properties
def topology(faces, num_vertices):
    """-> dict: euler (V - E + F over the vertices the faces use), closed (every directed edge once, its reverse once),
    boundary (the directed edges without a reverse), duplicates (directed edges that appear twice)"""
    f = faces.astype(np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = d[:, 0] * (num_vertices + 1) + d[:, 1]
    rev = d[:, 1] * (num_vertices + 1) + d[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    lonely = d[~np.isin(rev, key)]
    und = np.unique(np.minimum(key, rev))
    used = len(np.unique(f))
    return {"euler": used - len(und) + len(f), "closed": bool(len(lonely) == 0 and (cnt == 1).all()), "boundary": lonely,
            "duplicates": int((cnt > 1).sum()), "used": used}


def _nonzero_rows(n):
    return (n[..., 0] != 0.0) | (n[..., 1] != 0.0) | (n[..., 2] != 0.0)


def kuhn_interpolant(s8, p):
    """the piecewise-linear interpolant of the Kuhn split of the unit cell at points p (P, 3): s8[c] the value at corner
    c = dx + 2 dy + 4 dz; the mesh of one cell is its zero set"""
    order = np.argsort(-p, axis=1, kind="stable")
    x = np.take_along_axis(p, order, 1)
    c1 = 1 << order[:, 0]
    c2 = c1 | (1 << order[:, 1])
    s8 = np.asarray(s8)
    return s8[0] * (1.0 - x[:, 0]) + s8[c1] * (x[:, 0] - x[:, 1]) + s8[c2] * (x[:, 1] - x[:, 2]) + s8[7] * x[:, 2]


def face_normals(vertices, faces):
    """un-normalised geometric normals (F, 3) and centroids (F, 3)"""
    a, b, c = (vertices[faces[:, i]] for i in range(3))
    return np.cross(b - a, c - a), (a + b + c) / 3.0


# ------------------------------------------------------------------------------------------------------- volume cases
SPHERE_DIMS, SPHERE_CENTRE, SPHERE_RADIUS = (13, 11, 10), np.array([6.1, 5.2, 4.6]), 3.7
TWO_CENTRES, TWO_RADIUS = (np.array([3.3, 4.1, 4.6]), np.array([9.2, 6.3, 4.9])), 2.4
HOLE = (slice(3, 6), slice(2, 6), slice(5, 9))                  # (z, y, x) block of invalid nodes of the holes case
PLANE_NORMAL = (0.925, -0.22, 0.31)                            # crosses every slab of the grid, so every chunk counts
PLANE_DIMS = (67, 65, 63)                                       # 1072 groups: more than one chunk of the second-level scan


def _sphere_field(dims, centres, radius):
    X = node_positions((0.0, 0.0, 0.0), 1.0, dims)
    dist = [np.sqrt(((X[0] - c[0]) ** 2 + (X[1] - c[1]) ** 2) + (X[2] - c[2]) ** 2) - radius for c in centres]
    return np.minimum.reduce(dist)


def _colour_field(dims):
    X = node_positions((0.0, 0.0, 0.0), 1.0, dims)
    return np.stack([(0.2 + 0.05 * X[0]).reshape(-1), (0.9 - 0.04 * X[1]).reshape(-1), (0.3 + 0.03 * X[2]).reshape(-1)], -1)


@functools.lru_cache(maxsize=None)
def volume_cases():
    """name -> arguments of extract(): volumes written directly (weight 2 everywhere unless said, min_weight 1.5)"""
    def mk(dims, s, weight=None, color=True, origin=(0.0, 0.0, 0.0), voxel=1.0):
        w = np.full(s.size, 2.0) if weight is None else weight.reshape(-1).astype(np.float64)
        rgb = _colour_field(dims) * w[:, None] if color else None
        return dict(tsdf_sum=s.reshape(-1) * w, weight_sum=w, rgb_sum=rgb, origin=origin, voxel=voxel, dims=dims, min_weight=1.5)

    sphere = _sphere_field(SPHERE_DIMS, [SPHERE_CENTRE], SPHERE_RADIUS)
    two = _sphere_field(SPHERE_DIMS, TWO_CENTRES, TWO_RADIUS)
    hole_w = np.full(sphere.shape, 2.0)
    hole_w[HOLE] = 0.0
    nx, ny, nz = PLANE_DIMS
    X = node_positions((-3.3, -3.1, -2.9), 0.1, PLANE_DIMS)
    nrm = np.array(PLANE_NORMAL)
    plane = ((nrm[0] * (X[0] - 0.013) + nrm[1] * (X[1] - 0.021)) + nrm[2] * (X[2] - 0.037)) / np.linalg.norm(nrm)
    g = np.random.default_rng(11)
    tiny = g.uniform(0.2, 1.0, (2, 2, 2)) * np.array([1, -1])[g.integers(0, 2, (2, 2, 2))]
    return {
        "sphere": mk(SPHERE_DIMS, sphere), "two_spheres": mk(SPHERE_DIMS, two), "holes": mk(SPHERE_DIMS, sphere, hole_w),
        "sphere_no_colour": mk(SPHERE_DIMS, sphere, color=False),
        "all_inside": mk(SPHERE_DIMS, -1.0 - 0.01 * np.abs(sphere)), "all_outside": mk(SPHERE_DIMS, 1.0 + 0.01 * np.abs(sphere)),
        "tiny": mk((2, 2, 2), tiny, origin=(0.3, -0.2, 1.1), voxel=0.7),
        "plane_67x65x63": mk(PLANE_DIMS, plane, origin=(-3.3, -3.1, -2.9), voxel=0.1),
    }


@functools.lru_cache(maxsize=None)
def volume_reference(name):
    out = extract(**volume_cases()[name])
    _freeze(out)
    return out


def _freeze(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)


def sign_pattern_volume(pattern):
    """a 2 x 2 x 2 grid whose node c (c = dx + 2 dy + 4 dz) is inside when bit c of `pattern` (0 .. 255) is set"""
    s = np.array([-(0.3 + 0.05 * c) if pattern >> c & 1 else 0.4 + 0.03 * c for c in range(8)])
    return dict(tsdf_sum=s * 2.0, weight_sum=np.full(8, 2.0), rgb_sum=None, origin=(0.0, 0.0, 0.0), voxel=1.0, dims=(2, 2, 2),
                min_weight=1.5)


# ------------------------------------------------------------------------------------------------------- integration cases
GRID = dict(origin=(-0.513, -0.407, 3.691), voxel=0.05, dims=(21, 17, 13), trunc=0.2)
SMALL_GRID = dict(origin=(-0.471, -0.373, 3.767), voxel=0.12, dims=(9, 7, 5), trunc=0.3)


@functools.lru_cache(maxsize=None)
def integration_cases():
    """name -> arguments of integrate() but the volumes, and min_weight of the extraction that follows"""
    sc = FC.scenes()

    def mk(s, grid=GRID, depth=None, weights=None, color=True, min_weight=1.5, **over):
        d = FC._depth(s) if depth is None else depth
        case = dict(depth=d, weights=weights, frames=FC.colours(s["frames"]) if color else None, poses=s["poses"], cams=s["cams"],
                    min_weight=min_weight, **grid)
        case.update(over)
        return case

    b = sc["k08"]
    g = np.random.default_rng(5)
    wts = g.uniform(0.5, 1.5, FC._depth(b).shape).astype(np.float32)
    zeros = wts.copy()
    zeros[g.random(wts.shape) < 0.2] = 0.0
    away = b["poses"].copy()
    away[2] = np.diag([-1.0, 1.0, -1.0]) @ away[2]
    step = FC._depth(b).copy()
    step[:, :, 16:] *= np.float32(1.03)                                     # half of every map 3 % deeper: a step in the volume
    odd = sc["odd"]
    many = mk(odd, SMALL_GRID)                                              # 258 views: two launches of the integration
    many.update({k: np.ascontiguousarray(np.concatenate([many[k]] * 86)) for k in ("depth", "frames", "poses", "cams")})
    return {
        "many_views": many,
        "k0_24x32": mk(sc["k0"]), "k08_24x32": mk(b), "k08_21x35_small": mk(sc["odd"], SMALL_GRID),
        "k08_21x35": mk(sc["odd"]), "weights": mk(b, weights=wts, min_weight=1.25), "weights_zeros": mk(b, weights=zeros, min_weight=1.25),
        "no_frames": mk(b, color=False), "facing_away": mk(b, poses=away), "all_zero": mk(b, depth=np.zeros_like(FC._depth(b))),
        "depth_step": mk(b, depth=step), "holes": mk(b, depth=FC._holes(FC._depth(b))),
    }


def run_integration(case, first=0, last=None, volumes=None):
    """the views [first, last) of a case integrated onto `volumes` (default: zeroed ones)"""
    S = case["depth"].shape[0]
    last = S if last is None else last
    vol = empty_volume(case["dims"], case["frames"] is not None) if volumes is None else volumes
    sl = slice(first, last)
    return integrate(case["depth"][sl], None if case["weights"] is None else case["weights"][sl],
                     None if case["frames"] is None else case["frames"][sl], case["poses"][sl], case["cams"][sl], case["origin"],
                     case["voxel"], case["dims"], case["trunc"], *vol)


@functools.lru_cache(maxsize=None)
def integration_reference(name):
    """-> dict: tsdf_sum, weight_sum, rgb_sum, the extraction's outputs and all margins -- computed once, never modified"""
    case = integration_cases()[name]
    tsdf, wsum, rgb, mg = run_integration(case)
    out = extract(tsdf, wsum, rgb, case["origin"], case["voxel"], case["dims"], case["min_weight"])
    out.update(tsdf_sum=tsdf, weight_sum=wsum, rgb_sum=rgb)
    out["margins"] = dict(out["margins"], **mg)
    _freeze(out)
    return out


TRUTH_CASES = ("k0_24x32", "k08_24x32")
# measured on the restatement (tests/test_meshing_host.py prints them) over TRUTH_CASES, true depth maps
# rounded to float32, voxel 0.05, truncation 0.2: median and largest distance of a vertex from the scene's plane.  The CPU and
# the GPU tests assert 2 x these.
TRUTH_MEDIAN, TRUTH_LARGEST = 3.353e-3, 8.230e-3
