"""The yardstick of the nearest-neighbour tests: vggsfm_amd_nn.h restated in NumPy over ALL PAIRS -- no grid, no tree, no
candidate cells (that absence is what checks the kernel's structure) -- and the seeded cases.  Every expression stands in
the header's order, so the GPU tests compare bits.  The grid's own maps (cell ids, a query's range of cells, a face's box)
are restated too, for the host test that every accepted pair lies inside the kernel's candidate cells."""
import functools
import math

import numpy as np

from tests import render_cases as RC

INF = float("inf")
AXIS_LIMIT = 2.0 ** 40
STATS_GROUPS = 256
QUERY_CHUNK = 256


# ------------------------------------------------------------------------------------------------------- the grid
def default_box(points, cell):
    """origin, dims of the finite points' box (what PointGrid / TriangleGrid take without one)"""
    ok = np.isfinite(points).all(1) if len(points) else np.zeros(0, bool)
    if not ok.any():
        return [0.0] * 3, [1, 1, 1]
    lo, hi = points[ok].min(0), points[ok].max(0)
    return [float(v) for v in lo], [int(math.floor((float(h) - float(l)) / cell)) + 1 for l, h in zip(lo, hi)]


def axis_cells(coords, origin, cell, dims, shift=0.0):
    """c_a per axis (…,3) int64: clamp(floor((p - o) / cell) + shift, 0, dims - 1); the caller masks non-finite rows"""
    with np.errstate(all="ignore"):
        t = np.floor((coords - np.asarray(origin)) / cell) + shift
    t = np.where(np.isnan(t), -1.0, t)
    return np.clip(t, 0.0, np.asarray(dims, np.float64) - 1.0).astype(np.int64)


def cell_ids(points, origin, cell, dims):
    c = axis_cells(points, origin, cell, dims)
    ids = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    return np.where(np.isfinite(points).all(1), ids, -1).astype(np.int32)


def query_range(queries, r, origin, cell, dims):
    """lo, hi (M,3): the header's candidate cells per axis, margin and whole-axis rule included"""
    with np.errstate(all="ignore"):
        lo = axis_cells(queries - r, origin, cell, dims, -1.0)
        hi = axis_cells(queries + r, origin, cell, dims, 1.0)
        whole = ~((np.abs(queries) < AXIS_LIMIT * cell) & (r < AXIS_LIMIT * cell))
    return np.where(whole, 0, lo), np.where(whole, np.asarray(dims) - 1, hi)


# -------------------------------------------------------------------------------------------------- nearest point
def _d2(q, p):
    """((dx dx) + (dy dy)) + dz dz of queries (m,3) against points (n,3) -> (m,n)"""
    with np.errstate(all="ignore"):
        dx, dy, dz = (q[:, None, a] - p[None, :, a] for a in range(3))
        return ((dx * dx) + (dy * dy)) + dz * dz


def nearest_point(points, queries, max_dist, exclude_self=False):
    """-> dict index, dist2, count, and the margins: gap_best (the smallest (second - best) / r2 over the queries with two
    accepted candidates), gap_r2 (the smallest |d2 - r2| / r2 over all pairs), accepted (list of (query, point) index arrays)"""
    points, queries = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(queries, np.float64).reshape(-1, 3)
    r2 = float(max_dist) * float(max_dist)
    M, N = len(queries), len(points)
    index, dist2, count = np.full(M, -1, np.int32), np.full(M, INF), np.zeros(M, np.int32)
    gap_best, gap_r2, pairs = INF, INF, []
    candidate = np.isfinite(points).all(1)
    for s in range(0, M, QUERY_CHUNK):
        q = queries[s:s + QUERY_CHUNK]
        d2 = _d2(q, points)
        ok = candidate[None] & np.isfinite(q).all(1)[:, None]
        if exclude_self:
            ok = ok & (np.arange(s, s + len(q))[:, None] != np.arange(N)[None])
        with np.errstate(invalid="ignore"):
            acc = ok & (d2 <= r2)
        if N:
            masked = np.where(acc, d2, INF)
            best = masked.min(1)
            arg = masked.argmin(1)                                   # the first = the lowest index among equal d2
            has = acc.any(1)
            index[s:s + len(q)] = np.where(has, arg, -1)
            dist2[s:s + len(q)] = np.where(has, best, INF)
            count[s:s + len(q)] = acc.sum(1)
            if N > 1:
                second = np.partition(masked, 1, axis=1)[:, 1]
                two = np.isfinite(second)
                if two.any():
                    gap_best = min(gap_best, float(((second[two] - best[two]) / r2).min()))
            if ok.any():
                gap_r2 = min(gap_r2, float((np.abs(d2[ok] - r2) / r2).min()))
            qi, pi = np.nonzero(acc)
            pairs.append((qi + s, pi))
    qi = np.concatenate([p[0] for p in pairs]) if pairs else np.zeros(0, np.int64)
    pi = np.concatenate([p[1] for p in pairs]) if pairs else np.zeros(0, np.int64)
    return dict(index=index, dist2=dist2, count=count, gap_best=gap_best, gap_r2=gap_r2, accepted=(qi, pi))


# ----------------------------------------------------------------------------------------------- nearest triangle
def valid_faces(vertices, faces):
    """the header's skip rule -> (F,) bool and the triangles (F,3,3) (garbage where invalid)"""
    V, F = len(vertices), len(faces)
    f = faces.astype(np.int64)
    ok = ((f >= 0) & (f < V)).all(1) if F else np.zeros(0, bool)
    ok = ok & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    tri = np.zeros((F, 3, 3))
    tri[ok] = vertices[f[ok]]
    ok = ok & np.isfinite(tri).all((1, 2))
    tri[~ok] = 0.0
    ab, ac = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    n0 = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
    n1 = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
    n2 = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    return ok & (((n0 * n0) + (n1 * n1)) + n2 * n2 > 0.0), tri


def face_boxes(tri, origin, cell, dims):
    """lo, hi (F,3): the cells a (valid) face is registered in"""
    return axis_cells(tri.min(1), origin, cell, dims), axis_cells(tri.max(1), origin, cell, dims)


REGIONS = ("A", "B", "AB", "C", "AC", "BC", "interior")


def closest_points(tri, q):
    """Ericson 5.1.5 in the header's order for triangles (F,3,3) and queries (m,3) -> x (m,F,3), region (m,F) int"""
    dot = lambda x, y: ((x[..., 0] * y[..., 0]) + (x[..., 1] * y[..., 1])) + x[..., 2] * y[..., 2]
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    p = q[:, None]
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        ap, bp, cp = p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc = (d1 * d4) - (d3 * d2)
        vb = (d5 * d2) - (d1 * d6)
        va = (d3 * d6) - (d5 * d4)
        e, f = d4 - d3, d5 - d6
        tests = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e >= 0) & (f >= 0)]
        v_ab, w_ac, w_bc = d1 / (d1 - d3), d2 / (d2 - d6), e / (e + f)
        den = 1.0 / ((va + vb) + vc)
        v, w = vb * den, vc * den
        points = [a + 0 * p, b + 0 * p, a + v_ab[..., None] * ab, c + 0 * p, a + w_ac[..., None] * ac,
                  b + w_bc[..., None] * (c - b), (a + ab * v[..., None]) + ac * w[..., None]]
    region = np.full(tests[0].shape, 6)
    for k in range(5, -1, -1):
        region = np.where(tests[k], k, region)
    x = np.zeros(region.shape + (3,))
    for k in range(7):
        x = np.where((region == k)[..., None], points[k], x)
    return x, region


def nearest_face(vertices, faces, queries, max_dist):
    """-> dict face, dist2, closest, region (of the winner, -1 = none), gap_best (to the best face that shares no vertex
    with the winner), gap_r2, accepted"""
    vertices, queries = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(queries, np.float64).reshape(-1, 3)
    r2 = float(max_dist) * float(max_dist)
    ok, tri = valid_faces(vertices, faces)
    M, F = len(queries), len(faces)
    face, dist2 = np.full(M, -1, np.int32), np.full(M, INF)
    closest, region = np.full((M, 3), np.nan), np.full(M, -1)
    gap_best, gap_r2, pairs = INF, INF, []
    for s in range(0, M, QUERY_CHUNK):
        q = queries[s:s + QUERY_CHUNK]
        if not F:
            break
        x, reg = closest_points(tri, q)
        with np.errstate(all="ignore"):
            dx, dy, dz = (q[:, None, a] - x[..., a] for a in range(3))
            d2 = ((dx * dx) + (dy * dy)) + dz * dz
            cand = ok[None] & np.isfinite(q).all(1)[:, None]
            acc = cand & (d2 <= r2)
        masked = np.where(acc, d2, INF)
        best, arg, has = masked.min(1), masked.argmin(1), acc.any(1)
        rows = np.arange(len(q))
        face[s:s + len(q)] = np.where(has, arg, -1)
        dist2[s:s + len(q)] = np.where(has, best, INF)
        closest[s:s + len(q)] = np.where(has[:, None], x[rows, arg], np.nan)
        region[s:s + len(q)] = np.where(has, reg[rows, arg], -1)
        if F > 1:
            # the runner-up among the faces that share NO vertex with the winner: two faces tie by construction wherever the
            # closest point lies on their common edge or vertex (the lower index wins, in the kernel by the same arithmetic)
            fw = faces[arg].astype(np.int64)
            adjacent = (faces.astype(np.int64)[None, :, :, None] == fw[:, None, None, :]).any((2, 3))
            second = np.where(adjacent, INF, masked).min(1)
            two = np.isfinite(second) & has
            if two.any():
                gap_best = min(gap_best, float(((second[two] - best[two]) / r2).min()))
        if cand.any():
            gap_r2 = min(gap_r2, float((np.abs(d2[cand] - r2) / r2).min()))
        qi, fi = np.nonzero(acc)
        pairs.append((qi + s, fi))
    qi = np.concatenate([p[0] for p in pairs]) if pairs else np.zeros(0, np.int64)
    fi = np.concatenate([p[1] for p in pairs]) if pairs else np.zeros(0, np.int64)
    return dict(face=face, dist2=dist2, closest=closest, region=region, gap_best=gap_best, gap_r2=gap_r2, accepted=(qi, fi),
                valid=ok, triangles=tri)


# ----------------------------------------------------------------------------------------------------- statistics
def distance_stats(dist2, thresholds):
    """found, [below_k], and the two sums by math.fsum (the GPU sums are compared to these within the bound that holds for
    every order of summation)"""
    found = np.isfinite(dist2)
    d = np.sqrt(dist2[found])
    return int(found.sum()), [int((d < t).sum()) for t in thresholds], math.fsum(d.tolist()), math.fsum(dist2[found].tolist())


def radius_outlier_mask(points, radius, min_neighbors):
    return nearest_point(points, points, radius, exclude_self=True)["count"] >= min_neighbors


# ---------------------------------------------------------------------------------------------------- point cases
ORIGIN, CELL, DIMS = [-1.25, 0.5, 2.0], 0.5, [5, 3, 2]        # a 5 x 3 x 2 grid; origin + k cell is exact in binary
CELL_COUNTS = (0, 1, 63, 64, 65, 700)                         # points per cell, interleaved over the 30 cells


def _main_points(g):
    """the points of the 5 x 3 x 2 grid: cell i holds CELL_COUNTS[i % 6] points strictly inside it, the rows shuffled"""
    parts = []
    for i in range(30):
        c = np.array([i % 5, (i // 5) % 3, i // 15], np.float64)
        n = CELL_COUNTS[i % 6]
        parts.append(np.asarray(ORIGIN) + (c + g.uniform(0.01, 0.99, (n, 3))) * CELL)
    p = np.concatenate(parts)
    return p[g.permutation(len(p))]


def _box_queries(g, m, grow=0.3):
    lo = np.asarray(ORIGIN) - grow * CELL
    hi = np.asarray(ORIGIN) + (np.asarray(DIMS) + grow) * CELL
    return g.uniform(lo, hi, (m, 3))


@functools.lru_cache(maxsize=None)
def point_cases():
    """name -> dict points, queries, cell, origin, dims (None: the default box), max_dist, exclude_self, tie (the case is
    about ties: the gap floors do not apply)"""
    g = np.random.default_rng(34)
    main = _main_points(g)
    out = {}

    def add(name, points, queries, max_dist, cell=CELL, origin=ORIGIN, dims=DIMS, exclude_self=False, tie=False):
        out[name] = dict(points=np.ascontiguousarray(points, np.float64).reshape(-1, 3),
                         queries=np.ascontiguousarray(queries, np.float64).reshape(-1, 3), cell=cell, origin=origin, dims=dims,
                         max_dist=max_dist, exclude_self=exclude_self, tie=tie)
    big = _box_queries(g, 3001)
    for tag, cells in (("r04", 0.4), ("r10", 1.0), ("r23", 2.3)):            # reach 3, 3 and 5 cells per axis (+ the margin)
        add(f"main_{tag}", main, big, cells * CELL)
    for m in (1, 255, 256, 257):
        add(f"m{m}", main, _box_queries(g, m), 1.0 * CELL)
    add("n0", np.zeros((0, 3)), _box_queries(g, 257), CELL)
    add("n1", main[:1], np.concatenate([_box_queries(g, 256), main[:1] + 0.01]), 2.3 * CELL)
    add("m0", main[:500], np.zeros((0, 3)), CELL)
    add("one_cell", g.uniform(0.0, 1.0, (300, 3)), g.uniform(-0.2, 1.2, (257, 3)), 0.4, cell=1.0, origin=[0.0, 0.0, 0.0],
        dims=[1, 1, 1])
    # points exactly on cell faces and on the box's border, every combination of k cell per axis
    k0, k1, k2 = np.meshgrid(np.arange(6), np.arange(4), np.arange(3), indexing="ij")
    lattice = np.asarray(ORIGIN) + np.stack([k0, k1, k2], -1).reshape(-1, 3) * CELL
    add("on_faces", np.concatenate([lattice, main[:200]]), _box_queries(g, 300), 1.0 * CELL)
    # points and queries outside an explicitly given box: they live in, and reach, the border cells
    centre = np.asarray(ORIGIN) + 0.5 * np.asarray(DIMS) * CELL
    add("outside", centre + g.uniform(-3.0, 3.0, (1500, 3)), centre + g.uniform(-3.5, 3.5, (700, 3)), 1.0 * CELL)
    add("default_box", centre + g.uniform(-3.0, 3.0, (900, 3)), centre + g.uniform(-3.5, 3.5, (300, 3)), 0.9, cell=0.7,
        origin=None, dims=None)
    # ties: duplicate points (the lowest index wins), queries ON a duplicated point, a query midway between two points
    dup = main[:400].copy()
    dup[10], dup[399], dup[250] = dup[3], dup[3], dup[7]
    pair = np.asarray(ORIGIN) + np.array([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25]])       # exact; the midpoint is exact too
    dup[20], dup[5] = pair[0], pair[1]
    ties_q = np.concatenate([dup[[3, 7, 10, 250]], [(pair[0] + pair[1]) / 2.0], dup[[3]] + [0.0, 0.125, 0.0], _box_queries(g, 60)])
    add("ties", dup, ties_q, 1.0 * CELL, tie=True)
    # NaN and inf among the points and the queries
    bad_p = main[:600].copy()
    bad_p[[0, 17, 300]] = [[np.nan, 0.6, 2.1], [0.1, np.inf, 2.2], [-np.inf, 0.7, np.nan]]
    bad_q = _box_queries(g, 200)
    bad_q[[0, 5, 199]] = [[np.nan, np.nan, np.nan], [0.0, 1.0, np.inf], [-np.inf, 1.0, 2.5]]
    add("nonfinite", bad_p, bad_q, 1.0 * CELL, origin=None, dims=None)
    cloud = main[:1000]
    add("self", cloud, cloud, 0.4 * CELL, exclude_self=True)
    return out


def box_of(case):
    if case["origin"] is not None:
        return case["origin"], case["dims"]
    return default_box(case["points"] if "points" in case else case["vertices"], case["cell"])


@functools.lru_cache(maxsize=None)
def point_reference(name):
    c = point_cases()[name]
    return nearest_point(c["points"], c["queries"], c["max_dist"], c["exclude_self"])


# ------------------------------------------------------------------------------------------------- triangle cases
SPHERE_R = 1.5
REGION_TRIANGLE = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.5, 1.5, 0.25]])


def octahedron_sphere(levels=3, radius=SPHERE_R):
    """an octahedron subdivided `levels` times, every vertex pushed onto the sphere: 8 x 4^levels faces"""
    v = [(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = (np.asarray(v[i]) + np.asarray(v[j])) / 2.0
                v.append(tuple(m / np.linalg.norm(m)))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=1, keepdims=True) * radius, np.asarray(f, np.int32)


def skippable_mesh():
    """one good face (row 8) and every face the rule skips"""
    nan = float("nan")
    v = np.array([[-0.4, -0.3, 0.1], [0.5, -0.2, 0.3], [0.1, 0.4, 0.2],          # 0 1 2: the good face
                  [-0.2, -0.1, 0.8], [-0.2, -0.1, 0.8], [0.3, 0.1, 0.7],         # 3 4 5: rows 3 and 4 coincide: zero area
                  [0.1, nan, 0.5], [0.2, 0.2, np.inf],                            # 6 7: non-finite vertices
                  [0.0, 0.0, 1.0], [0.25, 0.25, 1.0], [0.5, 0.5, 1.0]])           # 8 9 10: collinear: zero area
    f = np.array([[0, 1, 1], [3, 4, 5], [0, 1, 11], [0, -1, 2], [0, 6, 2], [7, 1, 2], [8, 9, 10], [2, 2, 2], [0, 1, 2],
                  [1, 0, 2 ** 31 - 1], [-(2 ** 31), 1, 2]], np.int32)
    return v, f


def region_queries():
    """queries against REGION_TRIANGLE, one or more per region of Ericson's, with the expected label"""
    a, b, c = REGION_TRIANGLE
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n)
    out = [(a - 0.3 * (b - a) - 0.2 * (c - a) + 0.1 * n, "A"), (b + 0.4 * (b - a) + 0.1 * (b - c) - 0.2 * n, "B"),
           (c + 0.3 * (c - a) + 0.3 * (c - b) + 0.05 * n, "C"),
           (a + 0.5 * (b - a) + 0.2 * (c - a) + 0.3 * n, "interior"), (a + 0.25 * (b - a) + 0.25 * (c - a) - 0.4 * n, "interior")]
    for (p, q, r), label in (((a, b, c), "AB"), ((a, c, b), "AC"), ((b, c, a), "BC")):
        e = q - p
        outward = np.cross(e, n)                                 # in the triangle's plane, across the edge, away from r
        outward = outward if outward @ (r - p) < 0 else -outward
        out.append((p + 0.6 * e + 0.3 * outward / np.linalg.norm(outward) + 0.15 * n, label))
    return np.array([o[0] for o in out]), [o[1] for o in out]


@functools.lru_cache(maxsize=None)
def triangle_cases():
    """name -> dict vertices, faces, queries, cell, origin, dims, max_dist"""
    g = np.random.default_rng(35)
    out = {}

    def add(name, vertices, faces, queries, max_dist, cell, origin=None, dims=None):
        out[name] = dict(vertices=np.ascontiguousarray(vertices, np.float64).reshape(-1, 3),
                         faces=np.ascontiguousarray(faces, np.int32).reshape(-1, 3),
                         queries=np.ascontiguousarray(queries, np.float64).reshape(-1, 3), cell=cell, origin=origin, dims=dims,
                         max_dist=max_dist, tie=False)
    pv, pf = RC.plane_mesh()
    on = np.stack([g.uniform(-1.9, 1.9, 600), g.uniform(-1.5, 1.5, 600)], -1)
    pq = np.concatenate([on, (RC.PLANE[0] + RC.PLANE[1] * on[:, 0] + RC.PLANE[2] * on[:, 1] + g.uniform(-0.35, 0.35, 600))[:, None]], 1)
    add("plane", pv, pf, pq, 0.3, 0.2)
    add("plane_257", pv, pf, pq[:257], 0.2, 0.2)
    add("plane_255", pv, pf, pq[300:555], 0.46, 0.2, origin=[-1.0, -1.0, 1.5], dims=[9, 7, 4])      # a box smaller than the mesh
    sv, sf = octahedron_sphere()
    d = g.standard_normal((400, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sq = d * g.uniform(0.8, 1.35, (400, 1)) * SPHERE_R
    add("sphere", sv, sf, sq, 0.9, 0.3)
    kv, kf = skippable_mesh()
    kq = np.concatenate([g.uniform(-0.6, 0.7, (120, 3)), [[np.nan, 0.0, 0.0], [0.0, np.inf, 0.1]]])
    add("skippable", kv, kf, kq, 0.8, 0.25)
    # one face far larger than a cell among small ones
    small_v, small_f = octahedron_sphere(1, 0.2)
    lv = np.concatenate([[[-1.5, -1.2, 0.31], [1.6, -1.0, -0.27], [0.1, 1.7, 0.43]], small_v + [0.3, 0.2, 0.5]])
    lf = np.concatenate([[[0, 1, 2]], small_f + 3]).astype(np.int32)
    add("large_face", lv, lf, g.uniform(-1.7, 1.8, (300, 3)) * [1.0, 1.0, 0.5], 0.35, 0.1)
    add("f0", pv, np.zeros((0, 3), np.int32), pq[:257], 0.3, 0.2)
    add("f1", pv, pf[:1], pq[:255], 2.5, 0.5)
    rq, _ = region_queries()
    add("regions", REGION_TRIANGLE, [[0, 1, 2]], rq, 1.5, 0.5)
    return out


@functools.lru_cache(maxsize=None)
def triangle_reference(name):
    c = triangle_cases()[name]
    return nearest_face(c["vertices"], c["faces"], c["queries"], c["max_dist"])


def sampled_distance(tri, queries, n=48):
    """min over barycentric samples (n + 1)(n + 2) / 2 per triangle of the distance: an upper bound of the true distance,
    within (longest edge) / n of it -> (M,) and that slack"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    keep = i + j <= n
    u, v = i[keep] / n, j[keep] / n
    pts = tri[:, None, 0] + u[None, :, None] * (tri[:, None, 1] - tri[:, None, 0]) + v[None, :, None] * (tri[:, None, 2] - tri[:, None, 0])
    pts = pts.reshape(-1, 3)
    best = np.full(len(queries), INF)
    for s in range(0, len(pts), 65536):
        d = np.linalg.norm(queries[:, None] - pts[None, s:s + 65536], axis=-1).min(1)
        best = np.minimum(best, d)
    edges = np.linalg.norm(tri - np.roll(tri, 1, axis=1), axis=-1).max()
    return best, float(edges) / n
