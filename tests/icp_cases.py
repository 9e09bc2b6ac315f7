"""The yardstick of the ICP tests: vggsfm_amd_icp.h restated in NumPy over ALL PAIRS -- no grid, no candidate cells -- in
float64 and, with dtype=numpy.longdouble, in extended precision: the step (correspondences, residuals, Jacobian rows, normal
equations), the update (Jacobi-scaled Cholesky, Rodrigues, composition), the whole loop, and the radius normals; and the
seeded cases.  The correspondences follow the header's expressions in the header's order, so the GPU tests compare the
indices and the count bit for bit; the sums are compared within the bound that holds for any order of summation."""
import functools
import math

import numpy as np

from tests import nearest_cases as NC
from tests import render_cases as RC

INF = float("inf")
GROUPS, BLOCK, WORDS = 512, 256, 40
PIVOT_MIN = 1e-12
STATUS = ("running", "converged", "too few", "degenerate")
CHUNK = 256


# ---------------------------------------------------------------------------------------------------- transforms
def rotation(axis, degrees, dtype=np.float64):
    a = np.asarray(axis, dtype)
    a = a / np.sqrt((a * a).sum())
    th = dtype(degrees) * dtype(np.pi if dtype is np.float64 else np.arctan(dtype(1)) * 4) / dtype(180)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype)
    return np.eye(3, dtype=dtype) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def apply(T, p):
    """x_i = (s (((R_i0 p_0) + (R_i1 p_1)) + R_i2 p_2)) + t_i in the dtype of T"""
    s, R, t = T
    p = p.astype(R.dtype)
    return np.stack([(s * (((R[i, 0] * p[:, 0]) + (R[i, 1] * p[:, 1])) + R[i, 2] * p[:, 2])) + t[i] for i in range(3)], -1)


def invert(T):
    s, R, t = T
    return 1.0 / s, R.T, -(R.T @ t) / s


def transform_error(T, truth):
    """max over |s - s*|, |R - R*|, |t - t*| as a float"""
    return float(max(abs(T[0] - truth[0]), np.abs(T[1] - truth[1]).max(), np.abs(T[2] - truth[2]).max()))


# ---------------------------------------------------------------------------------------------- correspondences
def _dot(x, y):
    return ((x[..., 0] * y[..., 0]) + (x[..., 1] * y[..., 1])) + x[..., 2] * y[..., 2]


def nearest_points(points, x, r2):
    """the rule of vggsfm_amd_nn.h over all pairs, in the dtype of x -> index (M,) int32, y (M,3), gap_best, gap_r2"""
    M, N = len(x), len(points)
    index, y = np.full(M, -1, np.int32), np.zeros((M, 3), x.dtype)
    gap_best, gap_r2 = INF, INF
    cand = np.isfinite(points).all(1)
    if not N or not cand.any():
        return index, y, gap_best, gap_r2
    P = points.astype(x.dtype)
    for s in range(0, M, CHUNK):
        q = x[s:s + CHUNK]
        with np.errstate(all="ignore"):
            dx, dy, dz = (q[:, None, a] - P[None, :, a] for a in range(3))
            d2 = ((dx * dx) + (dy * dy)) + dz * dz
            ok = cand[None] & np.isfinite(q).all(1)[:, None]
            acc = ok & (d2 <= r2)
        masked = np.where(acc, d2, INF)
        arg, has = masked.argmin(1), acc.any(1)
        index[s:s + len(q)] = np.where(has, arg, -1)
        y[s:s + len(q)] = np.where(has[:, None], P[arg], 0)
        if N > 1:
            part = np.partition(masked, 1, axis=1)
            two = np.isfinite(part[:, 1].astype(np.float64))
            if two.any():
                gap_best = min(gap_best, float(((part[two, 1] - part[two, 0]) / r2).min()))
        if ok.any():
            gap_r2 = min(gap_r2, float((np.abs(d2[ok] - r2) / r2).min()))
    return index, y, gap_best, gap_r2


def nearest_faces(vertices, faces, x, r2, winners=None):
    """the rule of vggn_nearest_face over all pairs -> face (M,) int32, y (M,3), n (M,3) unit face normals, gaps.  winners:
    the faces are given (-1 = none) and only y and n are computed, in the dtype of x"""
    M, F = len(x), len(faces)
    face, y, n = np.full(M, -1, np.int32), np.zeros((M, 3), x.dtype), np.zeros((M, 3), x.dtype)
    gap_best, gap_r2 = INF, INF
    ok_face, tri = NC.valid_faces(vertices, faces)
    if not F or not ok_face.any():
        return face, y, n, gap_best, gap_r2
    T = tri.astype(x.dtype)
    for s in range(0, M, CHUNK):
        q = x[s:s + CHUNK]
        c, _ = NC.closest_points(T, q)
        with np.errstate(all="ignore"):
            dx, dy, dz = (q[:, None, a] - c[..., a] for a in range(3))
            d2 = ((dx * dx) + (dy * dy)) + dz * dz
            cand = ok_face[None] & np.isfinite(q).all(1)[:, None]
            acc = cand & (d2 <= r2)
        masked = np.where(acc, d2, INF)
        arg, has = masked.argmin(1), acc.any(1)
        if winners is not None:
            arg, has = np.maximum(winners[s:s + len(q)], 0), winners[s:s + len(q)] >= 0
        rows = np.arange(len(q))
        face[s:s + len(q)] = np.where(has, arg, -1)
        y[s:s + len(q)] = np.where(has[:, None], c[rows, arg], 0)
        ab, ac = T[arg, 1] - T[arg, 0], T[arg, 2] - T[arg, 0]
        u = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                      ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], -1)
        with np.errstate(all="ignore"):
            n[s:s + len(q)] = np.where(has[:, None], u / np.sqrt(_dot(u, u))[:, None], 0)
        if F > 1:
            fw = faces[arg].astype(np.int64)
            adjacent = (faces.astype(np.int64)[None, :, :, None] == fw[:, None, None, :]).any((2, 3))
            second = np.where(adjacent, INF, masked).min(1)
            two = np.isfinite(second.astype(np.float64)) & has
            if two.any():
                gap_best = min(gap_best, float(((second[two] - masked.min(1)[two]) / r2).min()))
        if cand.any():
            gap_r2 = min(gap_r2, float((np.abs(d2[cand] - r2) / r2).min()))
    return face, y, n, gap_best, gap_r2


# ------------------------------------------------------------------------------------------------------- the step
def step(source, target, T, center, max_dist, metric, estimate_scale, loss=0, loss_scale=0.0, dtype=np.float64):
    """target: dict points (N,3) [+ normals (N,3)] or vertices, faces.  metric 0 point to point, 1 point to plane; loss 0 none,
    1 Huber, 2 Tukey.  -> dict H (7,7), g (7,), sum_w, sum_wr2, sum_r2, count, index (M,) int32 (-1: no pair kept), the same
    sums over the absolute values of their terms (abs_H, abs_g, ...), gap_best, gap_r2."""
    T = (dtype(T[0]), np.asarray(T[1], dtype), np.asarray(T[2], dtype))
    c = np.asarray(center, dtype)
    r2 = dtype(float(max_dist) * float(max_dist))
    with np.errstate(all="ignore"):
        x = apply(T, np.asarray(source, np.float64).reshape(-1, 3))
    # the winners are decided in float64, whatever the dtype of the sums: the rule is the header's
    with np.errstate(all="ignore"):
        x64 = x if dtype is np.float64 else apply((np.float64(T[0]), T[1].astype(np.float64), T[2].astype(np.float64)),
                                                  np.asarray(source, np.float64).reshape(-1, 3))
    r2_64 = float(max_dist) * float(max_dist)
    if "faces" in target:
        index, y, n, gap_best, gap_r2 = nearest_faces(target["vertices"], target["faces"], x64, r2_64)
        if dtype is not np.float64:
            _, y, n, _, _ = nearest_faces(target["vertices"], target["faces"], x, r2, winners=index)
        have_normal = True
    else:
        index, y, gap_best, gap_r2 = nearest_points(target["points"], x64, r2_64)
        y = y.astype(dtype)
        have_normal = target.get("normals") is not None
        n = np.zeros_like(x)
        if have_normal and len(target["points"]):
            n = np.asarray(target["normals"], np.float64)[np.maximum(index, 0)].astype(dtype)
    keep = index >= 0
    if have_normal:
        keep = keep & np.isfinite(n.astype(np.float64)).all(1)
    index = np.where(keep, index, -1).astype(np.int32)
    x, y, n = x[keep], y[keep], n[keep]
    e, z = x - y, x - c
    P = len(x)
    zero, one = np.zeros(P, dtype), np.ones(P, dtype)
    if metric == 1:
        r = _dot(n, e)[:, None]
        lam = _dot(n, z) if estimate_scale else zero
        J = np.stack([z[:, 1] * n[:, 2] - z[:, 2] * n[:, 1], z[:, 2] * n[:, 0] - z[:, 0] * n[:, 2], z[:, 0] * n[:, 1] - z[:, 1] * n[:, 0],
                      n[:, 0], n[:, 1], n[:, 2], lam], -1)[:, None, :]
        R2 = r[:, 0] * r[:, 0]
        rho = np.abs(r[:, 0])
    else:
        r = e
        l = z if estimate_scale else np.zeros_like(z)
        J = np.stack([np.stack([zero, z[:, 2], -z[:, 1], one, zero, zero, l[:, 0]], -1),
                      np.stack([-z[:, 2], zero, z[:, 0], zero, one, zero, l[:, 1]], -1),
                      np.stack([z[:, 1], -z[:, 0], zero, zero, zero, one, l[:, 2]], -1)], 1)
        R2 = _dot(e, e)
        rho = np.sqrt(R2)
    k = dtype(loss_scale)
    with np.errstate(all="ignore"):
        if loss == 1:
            w = np.where(rho <= k, one, k / np.where(rho > 0, rho, 1))
        elif loss == 2:
            q = rho / k
            v = 1 - (q * q)
            w = np.where(rho < k, v * v, zero)
        else:
            w = one
    wJ = w[:, None, None] * J
    terms_H = wJ[:, :, :, None] * J[:, :, None, :]
    terms_g = wJ * r[:, :, None]
    out = dict(H=terms_H.sum((0, 1)), g=terms_g.sum((0, 1)), sum_w=w.sum(), sum_wr2=(w * R2).sum(), sum_r2=R2.sum(), count=int(P),
               abs_H=np.abs(terms_H).sum((0, 1)), abs_g=np.abs(terms_g).sum((0, 1)), abs_w=np.abs(w).sum(),
               abs_wr2=np.abs(w * R2).sum(), abs_r2=R2.sum(), index=index, gap_best=gap_best, gap_r2=gap_r2, weights=w, rho=rho)
    return out


# ----------------------------------------------------------------------------------------------------- the update
def update(S, T, center, estimate_scale, min_correspondences=6, damping=0.0, dtype=np.float64):
    """-> (status, T', (|omega|, |tau|, lambda), delta (7,)) by the header's update; T' = T when the status is not running"""
    s, R, t = dtype(T[0]), np.asarray(T[1], dtype), np.asarray(T[2], dtype)
    c = np.asarray(center, dtype)
    n = 7 if estimate_scale else 6
    zero = np.zeros(7, dtype)
    if S["count"] < min_correspondences:
        return 2, (s, R, t), None, zero
    H, g = np.asarray(S["H"], dtype), np.asarray(S["g"], dtype)
    if not (np.diag(H)[:n] > 0).all():
        return 3, (s, R, t), None, zero
    d = 1 / np.sqrt(np.diag(H)[:n])
    A = (H[:n, :n] * d[:, None]) * d[None, :]
    A[np.arange(n), np.arange(n)] = 1 + dtype(damping)
    b = -(g[:n] * d)
    L = np.zeros((n, n), dtype)
    for j in range(n):
        p = A[j, j]
        for k in range(j):
            p = p - L[j, k] * L[j, k]
        if not p > PIVOT_MIN:
            return 3, (s, R, t), None, zero
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, n):
            a = A[j, i]
            for k in range(j):
                a = a - L[i, k] * L[j, k]
            L[i, j] = a / L[j, j]
    yv = np.zeros(n, dtype)
    for i in range(n):
        a = b[i]
        for k in range(i):
            a = a - L[i, k] * yv[k]
        yv[i] = a / L[i, i]
    delta = np.zeros(7, dtype)
    for i in range(n - 1, -1, -1):
        a = yv[i]
        for k in range(i + 1, n):
            a = a - L[k, i] * delta[k]
        delta[i] = a / L[i, i]
    delta[:n] = delta[:n] * d
    w, tau, lam = delta[:3], delta[3:6], delta[6]
    th2 = ((w[0] * w[0]) + (w[1] * w[1])) + w[2] * w[2]
    th = np.sqrt(th2)
    if th2 < 1e-8:
        Ac, Bc = 1 - th2 / 6, dtype(0.5) - th2 / 24
    else:
        h = np.sin(dtype(0.5) * th)
        Ac, Bc = np.sin(th) / th, (2 * (h * h)) / th2
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype)
    E = (np.eye(3, dtype=dtype) + Ac * K) + Bc * (np.outer(w, w) - th2 * np.eye(3, dtype=dtype))
    u = t - c
    Rn = np.array([[((E[i, 0] * R[0, j]) + (E[i, 1] * R[1, j])) + E[i, 2] * R[2, j] for j in range(3)] for i in range(3)], dtype)
    tn = np.array([(c[i] + (1 + lam) * (((E[i, 0] * u[0]) + (E[i, 1] * u[1])) + E[i, 2] * u[2])) + tau[i] for i in range(3)], dtype)
    return 0, (s * (1 + lam), Rn, tn), (th, np.sqrt(((tau[0] * tau[0]) + (tau[1] * tau[1])) + tau[2] * tau[2]), lam), delta


def run(source, target, max_dist, init, center, iterations, metric, estimate_scale, loss=0, loss_scale=0.0, tol=(1e-9, 1e-9, 1e-9),
        min_correspondences=6, damping=0.0, dtype=np.float64):
    """the whole loop -> dict status, iterations, T, transforms (the T after each update), history (per iteration: count,
    sum_w, sum_wr2, sum_r2, |omega|, |tau|, lambda), gap_best, gap_r2 (the smallest over the iterations)"""
    T = (dtype(init[0]), np.asarray(init[1], dtype), np.asarray(init[2], dtype))
    status, transforms, history, gb, gr = 0, [], [], INF, INF
    for _ in range(iterations):
        S = step(source, target, T, center, max_dist, metric, estimate_scale, loss, loss_scale, dtype)
        gb, gr = min(gb, S["gap_best"]), min(gr, S["gap_r2"])
        status, T, norms, _ = update(S, T, center, estimate_scale, min_correspondences, damping, dtype)
        if status:
            break
        transforms.append(T)
        history.append([S["count"], S["sum_w"], S["sum_wr2"], S["sum_r2"], *norms])
        if norms[0] <= tol[0] and norms[1] <= tol[1] and abs(norms[2]) <= tol[2]:
            status = 1
            break
    return dict(status=STATUS[status], iterations=len(transforms), T=T, transforms=transforms, history=history, gap_best=gb, gap_r2=gr)


# ---------------------------------------------------------------------------------------------------- the normals
def radius_normals(points, radius, min_neighbors=5, toward=None):
    """all pairs, numpy.linalg.eigh -> normal (N,3), curvature (N,), count (N,) int32, eigen_gap (N,) = (l1 - l0) / l2"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    N = len(points)
    r2 = float(radius) * float(radius)
    normal, curv, gap = np.full((N, 3), np.nan), np.full(N, np.nan), np.full(N, np.nan)
    count = np.zeros(N, np.int32)
    fin = np.isfinite(points).all(1)
    with np.errstate(all="ignore"):
        d2 = NC._d2(points, points)
        acc = fin[:, None] & fin[None] & (d2 <= r2)
    gap_r2 = float((np.abs(d2[fin][:, fin] - r2) / r2).min()) if fin.any() else INF
    for i in range(N):
        nb = points[acc[i]]
        count[i] = len(nb)
        if not fin[i] or len(nb) < min_neighbors:
            continue
        a = nb - nb.mean(0)
        l, V = np.linalg.eigh(a.T @ a / len(nb))
        v = V[:, 0] / np.linalg.norm(V[:, 0])
        if toward is not None:
            flip = v @ (np.asarray(toward, np.float64) - points[i]) < 0
        else:
            flip = v[np.nonzero(v)[0][0]] < 0
        normal[i], curv[i], gap[i] = -v if flip else v, l[0] / l.sum(), (l[1] - l[0]) / l[2]
    return dict(normal=normal, curvature=curv, count=count, eigen_gap=gap, gap_r2=gap_r2)


# -------------------------------------------------------------------------------------------------- the base scene
SPACING = 2.0 / 47.0
MAX_DIST = 0.15
TRANSLATION = np.array([0.03, -0.02, 0.025])


def surface(x, y):
    z = 0.15 * np.sin(2.1 * x) + 0.1 * np.cos(1.7 * y) + 0.08 * np.sin(1.3 * x * y + 0.4)
    fx = 0.15 * 2.1 * np.cos(2.1 * x) + 0.08 * 1.3 * y * np.cos(1.3 * x * y + 0.4)
    fy = -0.1 * 1.7 * np.sin(1.7 * y) + 0.08 * 1.3 * x * np.cos(1.3 * x * y + 0.4)
    n = np.stack([-fx, -fy, np.ones_like(x)], -1)
    return z, n / np.linalg.norm(n, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def base_scene():
    """the 48 x 48 jittered grid on [-1, 1]^2 lifted onto the surface -> points (2304,3), normals, and 1500 seeded rows"""
    g = np.random.default_rng(36)
    u = np.linspace(-1.0, 1.0, 48)
    X, Y = np.meshgrid(u, u, indexing="ij")
    X = X + g.uniform(-0.3, 0.3, X.shape) * SPACING
    Y = Y + g.uniform(-0.3, 0.3, Y.shape) * SPACING
    Z, n = surface(X, Y)
    points = np.ascontiguousarray(np.stack([X, Y, Z], -1).reshape(-1, 3))
    rows = np.sort(g.choice(len(points), 1500, replace=False))
    return points, np.ascontiguousarray(n.reshape(-1, 3)), rows


def truth(degrees, t_factor, scale):
    return float(scale), rotation([1.0, 2.0, 3.0], degrees), TRANSLATION * t_factor


def moved_source(T, rows=None):
    """the target points `rows` moved by the inverse of T: registering them to the target recovers T"""
    points, _, all_rows = base_scene()
    rows = all_rows if rows is None else rows
    return np.ascontiguousarray(apply(invert(T), points[rows]))


def box_center(points, cell):
    origin, dims = NC.default_box(points, cell)
    return [o + 0.5 * d * cell for o, d in zip(origin, dims)]


IDENTITY = (1.0, np.eye(3), np.zeros(3))


@functools.lru_cache(maxsize=None)
def trajectory_cases():
    """name -> dict source, target, truth, metric, estimate_scale, iterations, max_dist, cell, center, init: the starts from
    which the loop reaches the truth (point-to-plane at 4 degrees, point-to-point at 1 degree)"""
    points, normals, _ = base_scene()
    out = {}
    for name, (deg, tf, sc, metric, es) in dict(plane_rigid=(4.0, 1.0, 1.0, 1, False), plane_scale=(4.0, 1.0, 1.03, 1, True),
                                                point_rigid=(1.0, 0.3, 1.0, 0, False), point_scale=(1.0, 0.3, 1.005, 0, True)).items():
        T = truth(deg, tf, sc)
        out[name] = dict(source=moved_source(T), target=dict(points=points, normals=normals), truth=T, metric=metric,
                         estimate_scale=es, iterations=8, max_dist=MAX_DIST, cell=MAX_DIST, center=box_center(points, MAX_DIST),
                         init=IDENTITY, loss=0, loss_scale=0.0)
    return out


@functools.lru_cache(maxsize=None)
def trajectory_reference(name, extended=False):
    c = trajectory_cases()[name]
    return run(c["source"], c["target"], c["max_dist"], c["init"], c["center"], c["iterations"], c["metric"], c["estimate_scale"],
               dtype=np.longdouble if extended else np.float64)


def _perturbed(seed, m):
    """m source points near the base surface at a small known offset from the target: a step case's source and transform"""
    points, _, _ = base_scene()
    g = np.random.default_rng(seed)
    rows = np.sort(g.choice(len(points), m, replace=False)) if m else np.zeros(0, np.int64)
    T = truth(1.5, 0.5, 1.01)
    src = apply(invert(T), points[rows]) + g.normal(0.0, 0.004, (m, 3))
    start = (1.004, rotation([0.3, -1.0, 0.5], 0.7), np.array([0.004, 0.003, -0.005]))
    return np.ascontiguousarray(src), start


@functools.lru_cache(maxsize=None)
def step_cases():
    """name -> dict source, target, T, center, max_dist, cell, metric, estimate_scale, loss, loss_scale"""
    points, normals, _ = base_scene()
    cloud = dict(points=points, normals=normals)
    centre = box_center(points, MAX_DIST)
    out = {}

    def add(name, source, target, T, metric=1, estimate_scale=True, loss=0, loss_scale=0.0, max_dist=MAX_DIST, cell=MAX_DIST,
            center=None):
        pts = target["points"] if "points" in target else target["vertices"]
        out[name] = dict(source=np.ascontiguousarray(source, np.float64).reshape(-1, 3), target=target, T=T, metric=metric,
                         estimate_scale=estimate_scale, loss=loss, loss_scale=loss_scale, max_dist=max_dist, cell=cell,
                         center=box_center(pts, cell) if center is None else center)
    for m in (0, 1, 63, 64, 65, 255, 256, 257, 1500):
        src, T = _perturbed(100 + m, m)
        add(f"m{m}", src, cloud, T, center=centre)
    src, T = _perturbed(7, 700)
    add("n0", src, dict(points=np.zeros((0, 3)), normals=np.zeros((0, 3))), T, center=centre)
    add("none_within", src + [0.0, 0.0, 5.0], cloud, T, center=centre)
    for metric in (0, 1):
        for es in (False, True):
            for loss, k in ((0, 0.0), (1, 0.004), (2, 0.012)):
                add(f"metric{metric}_scale{int(es)}_loss{loss}", src, cloud, T, metric, es, loss, k, center=centre)
    add("point_to_point_no_normals", src, dict(points=points), T, metric=0, center=centre)
    # NaN / inf among the target points, the source points and the normals
    bp, bn, bs = points.copy(), normals.copy(), src.copy()
    bp[[5, 900]] = [[np.nan, 0.0, 0.0], [0.1, np.inf, 0.2]]
    bn[[17, 1200, 2000]] = [[np.nan, 0.0, 1.0], [0.0, np.inf, 0.0], [np.nan] * 3]
    bs[[0, 100, 699]] = [[np.nan] * 3, [0.0, np.inf, 0.1], [-np.inf, 0.0, 0.0]]
    add("nonfinite", bs, dict(points=bp, normals=bn), T, center=centre)
    # the mesh targets: section 33's jittered plane grid, section 34's subdivided octahedron
    g = np.random.default_rng(37)
    pv, pf = RC.plane_mesh()
    on = np.stack([g.uniform(-1.9, 1.9, 600), g.uniform(-1.5, 1.5, 600)], -1)
    pq = np.concatenate([on, (RC.PLANE[0] + RC.PLANE[1] * on[:, 0] + RC.PLANE[2] * on[:, 1] + g.uniform(-0.2, 0.2, 600))[:, None]], 1)
    small = (1.002, rotation([1.0, 0.2, -0.4], 0.5), np.array([0.01, -0.006, 0.008]))
    for metric in (0, 1):
        add(f"mesh_plane_metric{metric}", pq, dict(vertices=pv, faces=pf), small, metric, True, max_dist=0.3, cell=0.2)
    sv, sf = NC.octahedron_sphere()
    d = g.standard_normal((400, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sq = d * g.uniform(0.8, 1.35, (400, 1)) * NC.SPHERE_R
    add("mesh_sphere", sq, dict(vertices=sv, faces=sf), small, 1, True, 1, 0.1, max_dist=0.9, cell=0.3)
    add("mesh_f0", pq[:257], dict(vertices=pv, faces=np.zeros((0, 3), np.int32)), small, 1, True, max_dist=0.3, cell=0.2)
    return out


@functools.lru_cache(maxsize=None)
def step_reference(name, extended=False):
    c = step_cases()[name]
    return step(c["source"], c["target"], c["T"], c["center"], c["max_dist"], c["metric"], c["estimate_scale"], c["loss"],
                c["loss_scale"], np.longdouble if extended else np.float64)


NORMAL_RADIUS = 0.12


@functools.lru_cache(maxsize=None)
def normals_cases():
    points, _, _ = base_scene()
    bad = points[:600].copy()
    bad[[3, 77]] = [[np.nan, 0.0, 0.0], [0.0, 0.1, np.inf]]
    lonely = np.concatenate([points[:400], [[5.0, 5.0, 5.0], [5.01, 5.0, 5.0]]])
    return dict(surface=dict(points=points, radius=NORMAL_RADIUS, min_neighbors=5, toward=None),
                toward=dict(points=points, radius=NORMAL_RADIUS, min_neighbors=5, toward=[0.2, -0.3, 4.0]),
                nonfinite=dict(points=bad, radius=NORMAL_RADIUS, min_neighbors=5, toward=None),
                lonely=dict(points=lonely, radius=NORMAL_RADIUS, min_neighbors=5, toward=None))


@functools.lru_cache(maxsize=None)
def normals_reference(name):
    c = normals_cases()[name]
    return radius_normals(c["points"], c["radius"], c["min_neighbors"], c["toward"])
