"""The yardstick of the LO-RANSAC triangulation kernels (csrc/triangulate.hip) beyond the mild goldens: a table of hard
geometries and lane-structure edges, and ``oracle.geometry.triangulate_tracks_chunk`` restated once in ``np.longdouble``
(DLT matrices, smallest eigenvector by a cyclic Jacobi written with numpy operations -- numpy's linalg has no long double
--, cheirality, the pair / all-pairs triangulation angle, angular errors, the two LO rounds with stable descending
selection, ``residual_indicator`` with the chunk-global threshold, first maximum).

The same code evaluated in float64 -- made to follow the long-double run's selections, so that the two are compared
quantity by quantity -- gives ``dev64``: how far plain double arithmetic lands from long double.  Every bound below is built
from that, never from what the kernel produces.  ``dev64_lapack`` is the same run with the reference's own eigen-solver
(LAPACK ``eigh``) in place of the Jacobi: on badly scaled DLT matrices (scene units of 100, a scene far from the origin)
LAPACK is up to three decades less accurate than a Jacobi in the same precision, so the reference project's recorded
points are held to the bound built from ``dev64_lapack`` and the device to the tighter one built from ``dev64``.

The outputs are discontinuous in the decisions, so the reference also says per track whether a comparison is meaningful
(`admitted`); no case may leave out more than ``CAP`` of its tracks.

tests/test_triangulation_cases.py checks all of this by itself on the CPU and against the reference project's recorded
output (tests/golden/tri_regimes_*.npz, written by oracle/gen_golden_tri_regimes.py); tests/test_gpu_triangulation_regimes.py
compares the device with the recorded long-double results."""
import hashlib
import os

import numpy as np

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

CAP = 0.02                    # no case leaves out more than this share of its tracks (= essential_cases.CAP)
LO_NUM, MAX_ANGULAR_ERROR, MIN_TRI_ANGLE = 50, 2.0, 1.5          # the reference's defaults
MAX_RAD = MAX_ANGULAR_ERROR * (np.pi / 180)                       # the float64 number reference and kernel compare with
DELTA_FLOOR, MARGIN = 1e-9, 100.0     # delta = max(DELTA_FLOOR rad, MARGIN x largest float64-vs-long-double difference)
POINT_FLOOR = 1e-13                   # point bound = max(POINT_FLOOR, MARGIN x dev64 of the case)
THRESHOLD_RTOL = 1e-12                # per-chunk indicator thresholds, relative
GAP_MIN = 1e-12                       # (lambda_2 - lambda_1) / lambda_4 below which the eigenvector is not compared
EPS64 = float(np.finfo(np.float64).eps)

# pair_sweep: largest angle(v, v_ld) / (EPS64 lambda_4 / (lambda_2 - lambda_1)) that float64 LAPACK (np.linalg.eigh on the
# float64 DLT matrices) reaches over the inputs with a gap >= GAP_MIN, measured on the CPU by
# tests/test_triangulation_cases.py::test_pair_sweep_lapack_constant; the bound for the device is ten times that.
PAIR_C_LAPACK = 1.276
PAIR_C = 10 * PAIR_C_LAPACK
# Largest values measured on an MI355X, next to the rules that bound them; a measured value is never
# its own bound.  Points: the largest relative deviation over all cases (`forward`, bound 2.4e-9) and the largest share of
# its case's bound any case reaches (`viscount`); thresholds: `rethreshold` and `grid_stride_every`, relative; two-view
# eigenvector: largest angle / (EPS64 lambda_4 / gap) on the sweep and over all groups (`outl50`), bound PAIR_C.
POINT_MEASURED = 2.7e-12
POINT_BOUND_SHARE_MEASURED = 0.065
THRESHOLD_MEASURED = (2.6e-13, 1.5e-13)
PAIR_C_MEASURED = (0.153, 0.669)


# --- 4x4 symmetric eigen-solve in any dtype ----------------------------------------------------------------------------
def jacobi_eigh4(A, sweeps=20):
    """Cyclic Jacobi on a batch of symmetric 4x4 matrices (B,4,4) in A's dtype -> (eigenvalues (B,4) ascending,
    eigenvectors (B,4,4) in columns, same order; ties keep the lower index first)."""
    dt = A.dtype.type
    B = A.shape[0]
    a = [[A[:, i, j].copy() for j in range(4)] for i in range(4)]
    v = [[np.full(B, 1.0 if i == j else 0.0, dtype=A.dtype) for j in range(4)] for i in range(4)]
    one, tiny = dt(1), np.finfo(A.dtype).eps * dt(1e-4)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            off = sum(np.abs(a[p][q]) for p in range(3) for q in range(p + 1, 4))
            dsum = sum(np.abs(a[p][p]) for p in range(4))
            if not np.any(off > tiny * dsum):
                break
            for p in range(3):
                for q in range(p + 1, 4):
                    apq = a[p][q]
                    nz = apq != 0
                    theta = (a[q][q] - a[p][p]) / (2 * np.where(nz, apq, one))
                    t = np.where(theta >= 0, one, -one) / (np.abs(theta) + np.hypot(theta, one))
                    t = np.where(nz, t, 0 * one)
                    c = one / np.sqrt(t * t + one)
                    s = t * c
                    for k in range(4):
                        akp, akq = a[k][p], a[k][q]
                        a[k][p], a[k][q] = c * akp - s * akq, s * akp + c * akq
                    for k in range(4):
                        apk, aqk = a[p][k], a[q][k]
                        a[p][k], a[q][k] = c * apk - s * aqk, s * apk + c * aqk
                    a[p][q] = np.where(nz, 0 * one, a[p][q])
                    a[q][p] = a[p][q]
                    for k in range(4):
                        vkp, vkq = v[k][p], v[k][q]
                        v[k][p], v[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
    w = np.stack([a[k][k] for k in range(4)], -1)
    V = np.stack([np.stack(v[k], -1) for k in range(4)], -2)                   # (B,4,4)[row, column]
    order = np.argsort(np.where(np.isnan(w), np.inf, w), axis=-1, kind="stable")
    return np.take_along_axis(w, order, -1), np.take_along_axis(V, order[:, None, :], -1)


# --- the formulas of oracle/geometry.py in any dtype ---------------------------------------------------------------------
def _pi(dt):
    return np.arccos(dt(-1))


def unit_rays(tn):
    ph = np.concatenate([tn, np.ones_like(tn[..., :1])], -1)
    return ph / np.sqrt((ph * ph).sum(-1, keepdims=True))


def view_matrices(ext, rays):
    """ext (S,3,4), unit rays (B,S,3) -> T^T T of every view, T = P - r r^T P: (B,S,4,4)."""
    rp = np.einsum("bsi,sik->bsk", rays, ext)
    terms = ext[None] - rays[..., :, None] * rp[..., None, :]
    return np.einsum("bsij,bsik->bsjk", terms, terms)


def centres(ext):
    return -np.einsum("sji,sj->si", ext[:, :, :3], ext[:, :, 3])


def tri_angle_deg(r1sq, r2sq, bsq):
    dt = r1sq.dtype.type
    pi = _pi(dt)
    with np.errstate(all="ignore"):
        den = 2 * np.sqrt(r1sq * r2sq)
        nom = r1sq + r2sq - bsq
        bad = den <= dt(1e-12)
        c = np.clip(np.where(bad, dt(1), nom) / np.where(bad, dt(1), den), -1, 1)
        th = np.abs(np.arccos(c))
        return np.minimum(th, pi - th) * (180 / pi)


def max_pair_angle(cen, X):
    """Largest triangulation angle in degrees over all pairs of the S centres at X (...,3); -1 where X is not finite."""
    with np.errstate(all="ignore"):
        r = ((X[..., None, :] - cen) ** 2).sum(-1)
    best = np.full(X.shape[:-1], -1, dtype=X.dtype)
    for a in range(len(cen) - 1):
        bsq = ((cen[a + 1:] - cen[a]) ** 2).sum(-1)
        best = np.fmax(best, np.fmax.reduce(tri_angle_deg(r[..., a:a + 1], r[..., a + 1:], bsq), axis=-1))
    return best


def view_geometry(ext, rays, X):
    """X (B,C,3) against every view: angular error (B,C,S) (NaN where the reference's is), depth z and |R X + t|."""
    dt = X.dtype.type
    with np.errstate(all="ignore"):
        y = np.einsum("sij,bcj->bcsi", ext[:, :, :3], X) + ext[None, None, :, :, 3]
        n = np.sqrt((y * y).sum(-1))
        yn = y / np.maximum(n, dt(1e-12))[..., None]
        err = np.arccos(np.clip((rays[:, None] * yn).sum(-1), -1, 1))
    return err, y[..., 2], n


def _rel_depth(z, n):
    """z / |y| with the reference's decisions kept where it is undefined: z <= 0 fails, NaN passes."""
    with np.errstate(all="ignore"):
        return np.where(n > 0, z / n, np.where(z <= 0, -np.inf, np.inf)).astype(z.dtype)


def stable_desc(x):
    return np.argsort(-x, axis=-1, kind="stable")


def _solve(A, lapack=False):
    B = A.shape[:-2]
    V = np.linalg.eigh(A.reshape(-1, 4, 4))[1] if lapack else jacobi_eigh4(A.reshape(-1, 4, 4))[1]
    v0 = V[:, :, 0]
    with np.errstate(all="ignore"):
        X = v0[:, :3] / v0[:, 3:]
    return X.reshape(B + (3,))


def solve_chunk(ext, tn, ivc, pairs, dt=LD, follow=None, lo_num=LO_NUM, thres=None, lapack=False):
    """One reference chunk.  ext (S,3,4), tn (B,S,2), ivc (B,S) bool (True = the view does not count), pairs (H,2).
    Candidates are ordered [RANSAC 0..H-1 | LO1 | LO2].  With `follow` (the result of the long-double run) the selections
    and inlier sets that feed the LO rounds and the winner are taken from it, so that every quantity has its counterpart.
    The chunk threshold is rounded to float64 before it is used (it only scales the indicator), so that a run on some of the
    tracks, given the recorded threshold as `thres`, repeats the run on all of them bit for bit.
    `lapack` (float64 only): np.linalg.eigh, the reference's own eigen-solver, in place of the Jacobi."""
    ext, tn = ext.astype(dt), tn.astype(dt)
    B, S, _ = tn.shape
    H = len(pairs)
    lo1 = min(lo_num, H)
    lo2 = min(10, lo1)
    pi = _pi(dt)
    rays = unit_rays(tn)
    M = view_matrices(ext, rays)
    cen = centres(ext)
    vis = ~ivc
    i1, i2 = pairs[:, 0], pairs[:, 1]
    # ---- RANSAC: two-view DLT, cheirality in the two views, angle of the pair
    X0 = _solve(M[:, i1] + M[:, i2], lapack)                                                  # (B,H,3)
    err0, z0, n0 = view_geometry(ext, rays, X0)
    rd0 = _rel_depth(z0, n0)
    hh = np.arange(H)
    zr0 = np.minimum(rd0[:, hh, i1], rd0[:, hh, i2])
    with np.errstate(all="ignore"):
        ang0 = tri_angle_deg(((X0 - cen[i1]) ** 2).sum(-1), ((X0 - cen[i2]) ** 2).sum(-1), ((cen[i1] - cen[i2]) ** 2).sum(-1))
        ang0 = np.where(np.isnan(ang0), dt(-1), ang0)
        valid0 = (ang0 >= MIN_TRI_ANGLE) & ~((z0[:, hh, i1] <= 0) | (z0[:, hh, i2] <= 0))
        inl0 = valid0[:, :, None] & vis[:, None, :] & (err0 <= MAX_RAD)

    def refine(inl_prev, lo, order, mask):
        if order is None:
            order = stable_desc(inl_prev.sum(-1))[:, :lo]
            mask = np.take_along_axis(inl_prev, order[:, :, None], axis=1)
        X = _solve(np.einsum("bcs,bsij->bcij", mask.astype(dt), M), lapack)
        err, z, n = view_geometry(ext, rays, X)
        ang = max_pair_angle(cen, X)
        with np.errstate(all="ignore"):
            valid = (ang >= MIN_TRI_ANGLE) & ~(z <= 0).any(-1)
        zr = _rel_depth(z, n).min(-1)
        err = np.where(np.isfinite(err), err, 100 * pi)
        inl = valid[:, :, None] & vis[:, None, :] & (err <= MAX_RAD)
        return dict(X=X, err=err, ang=ang, zr=zr, valid=valid, inl=inl, order=order, mask=mask)

    f = follow or {}
    r1 = refine(inl0, lo1, f.get("order1"), f.get("mask1"))
    r2 = refine(r1["inl"], lo2, f.get("order2"), f.get("mask2"))
    X = np.concatenate([X0, r1["X"], r2["X"]], 1)
    err = np.concatenate([err0, r1["err"], r2["err"]], 1)
    valid = np.concatenate([valid0, r1["valid"], r2["valid"]], 1)
    inl = np.concatenate([inl0, r1["inl"], r2["inl"]], 1)
    # ---- residual_indicator: the reference adds pi to the errors of void hypotheses and views; NaN poisons the mean
    with np.errstate(all="ignore"):
        tot = err + np.where(valid, 0, pi)[:, :, None] + np.where(vis, 0, pi)[:, None, :]
        num = inl.sum(-1)
        emean = (inl.astype(dt) * tot).sum(-1) / num
    emean = np.where(np.isfinite(emean), emean, 2 * pi)
    own = dt(np.float64(emean.max() + dt(1e-6) if B else 2 * pi + dt(1e-6)))
    thres = own if thres is None else dt(thres)
    ind = (thres - emean) / thres + num.astype(dt)
    best = np.argmax(ind, axis=1) if follow is None else follow["best"]
    return dict(X=X, err=err, valid=valid, inl=inl, num=num, emean=emean, thres=own, best=best,
                ang=np.concatenate([ang0, r1["ang"], r2["ang"]], 1), zr=np.concatenate([zr0, r1["zr"], r2["zr"]], 1),
                order1=r1["order"], mask1=r1["mask"], order2=r2["order"], mask2=r2["mask"], H=H, lo1=lo1, lo2=lo2, vis=vis,
                ext=ext, rays=rays)


def _absdiff(a, b, where):
    with np.errstate(all="ignore"):
        d = np.abs(a.astype(LD) - b.astype(LD))
    d = d[where & np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


def rel_point_distance(X, X_ld, size):
    with np.errstate(all="ignore"):
        d = np.sqrt(((X.astype(LD) - X_ld.astype(LD)) ** 2).sum(-1))
        return (d / np.maximum(np.sqrt((X_ld.astype(LD) ** 2).sum(-1)), size)).astype(np.float64)


def stability(ld, delta):
    """Which decisions of a long-double chunk result can reach the track's output, and which of them lie within delta of
    their threshold.
    A hypothesis can reach the output when it is selected for the next round, or could be after the flips its near
    decisions allow (count with every near decision going its way >= count of the last one selected), or could then equal
    or beat the winner's count.
    `undefined`: an LO candidate solved from ONE view.  Its DLT matrix has a two-dimensional null space (the view's ray),
    so the point is an arbitrary point of that ray in any arithmetic, and so is its validity; it can have that one view as
    its inlier, or none.  Its quantities are not compared and it counts as reaching the output of a track whose winner has
    fewer than two inliers."""
    H, lo1, lo2 = ld["H"], ld["lo1"], ld["lo2"]
    B = len(ld["best"])
    ar = np.arange(B)
    ddeg = delta * 180 / np.pi
    vis3 = ld["vis"][:, None, :]
    undefined = np.concatenate([np.zeros((B, H), bool), ld["mask1"].sum(-1) == 1, ld["mask2"].sum(-1) == 1], 1)
    with np.errstate(all="ignore"):
        ang, zr, err = ld["ang"], ld["zr"], ld["err"]
        rob_valid = (ang >= MIN_TRI_ANGLE + ddeg) & (zr > delta)
        rob_invalid = ~(ang >= MIN_TRI_ANGLE - ddeg) | ~(zr > -delta)
        val_near = ~(rob_valid | rob_invalid)
        potential = np.where(rob_invalid, 0, (vis3 & (err <= MAX_RAD + delta)).sum(-1))
        near_err = (vis3 & (np.abs(err - MAX_RAD) <= delta)).sum(-1)
    unstable = ~rob_invalid & ((val_near & (potential > 0)) | (near_err > 0)) & ~undefined
    n_win = ld["num"][ar, ld["best"]]
    reach = potential >= n_win[:, None]
    for lo, order, first, count in ((lo1, ld["order1"], 0, H), (lo2, ld["order2"], H, lo1)):
        num = ld["num"][:, first:first + count]
        chosen = np.zeros((B, count), bool)
        np.put_along_axis(chosen, order, True, axis=1)
        last = np.take_along_axis(num, order[:, -1:], axis=1)
        reach[:, first:first + count] |= chosen | (potential[:, first:first + count] >= last)
    return dict(reach=reach, unstable=unstable, rob_invalid=rob_invalid, undefined=undefined, n_win=n_win)


def ray_can_win(ext, cen, rays, vis, view, size, n_win, e_win, delta):
    """Can some point of the ray of `view`, in front of every camera, be the winner of a track whose winner has n_win inliers
    at a mean error of e_win?  (More inliers, or as many at a mean error not above e_win + delta.)  float64, exhaustive:
    depths from 1e-3 to 1e3 scene sizes (beyond, no camera pair subtends MIN_TRI_ANGLE), log-spaced 2.7 % apart; every
    sample stands for the segment around it -- a point that moves by m is seen to move by at most m / distance from a
    camera, so every error is lowered by that much, with a factor 1.5 for the distance changing along the segment -- and
    the segments that pass are divided again by 256."""
    d = ext[view, :, :3].T @ rays[view]
    need = max(int(n_win), 1)
    if need > int(vis.sum()):
        return False

    def passes(t, half):
        y = (cen[view] + t[:, None] * d) @ ext[:, :, :3].transpose(0, 2, 1) + ext[:, None, :, 3]            # (S,T,3)
        n = np.maximum(np.sqrt((y * y).sum(-1)), 1e-300)
        margin = 1.5 * half * t[None] / n
        low = np.maximum(np.arccos(np.clip((rays[:, None] * y).sum(-1) / n, -1, 1)) - margin, 0)
        front = (y[..., 2] > -margin * n).all(0)
        low = np.sort(np.where(vis[:, None], low, np.inf), axis=0)
        cnt = (low <= MAX_RAD).sum(0)
        return front & ((cnt > n_win) | ((cnt >= need) & (low[:need].mean(0) <= e_win + delta)))

    ratio = 10 ** (6 / 512)
    t = size * 1e-3 * ratio ** np.arange(513)
    hit = np.nonzero(passes(t, np.sqrt(ratio) - 1))[0]
    for k0 in range(0, len(hit), 16):
        fine = (t[hit[k0:k0 + 16], None] * ratio ** np.linspace(-0.5, 0.5, 257)[None]).ravel()
        if passes(fine, (np.sqrt(ratio) - 1) / 256).any():
            return True
    return False


def decision_dev64(ld, f64):
    """Largest float64-vs-long-double difference of a quantity on which a decision that can reach the output is taken: the
    triangulation angle (radians), the relative depth z / |R X + t|, and the angular errors on the visible views.  The arc
    cosine's conditioning is 1 / sin(error) and the decision is taken at MAX_RAD, so errors count between half and twice
    MAX_RAD.  Hypotheses that are void by a margin of DELTA_FLOOR, and undefined ones, have no decision left."""
    st = stability(ld, DELTA_FLOOR)
    use = st["reach"] & ~st["rob_invalid"] & ~st["undefined"]
    with np.errstate(all="ignore"):
        band = (ld["err"] >= MAX_RAD / 2) & (ld["err"] <= 2 * MAX_RAD)
    return max(_absdiff(ld["err"], f64["err"], use[:, :, None] & ld["vis"][:, None, :] & band),
               _absdiff(ld["ang"], f64["ang"], use) * np.pi / 180, _absdiff(ld["zr"], f64["zr"], use))


def admit(ld, delta, point_bound, size):
    """Per track: (a) no decision that can reach the output within delta of its threshold, (b) every candidate whose
    indicator is within delta of the winner's yields the winner's mask (and, with point_bound, its point)."""
    st = stability(ld, delta)
    B = len(ld["best"])
    ar = np.arange(B)
    n_win, undefined = st["n_win"], st["undefined"]
    ok_a = ~(st["unstable"] & st["reach"]).any(1)
    # Undefined candidates.  With at most one visible view every mask is that view or nothing: the output is the same
    # whatever such a candidate does if a defined candidate has that one inlier as well.  Otherwise the candidate may be any
    # point of its ray: the track is admitted only if no point of the ray can be the winner.
    e_win = ld["emean"][ar, ld["best"]]
    single = (ld["num"] == 1) & ~undefined
    nvis = ld["vis"].sum(1)
    solved_from = np.concatenate([np.zeros((B, ld["H"], ld["vis"].shape[1]), bool), ld["mask1"], ld["mask2"]], 1)
    ray_view = np.argmax(solved_from, axis=2)
    ok_a &= ~undefined.any(1) | (nvis >= 2) | (single.any(1) & (n_win == 1))
    bb, cc = np.nonzero(undefined & ((nvis >= 2) & ok_a)[:, None])
    if len(bb):
        ext64, rays64 = ld["ext"].astype(np.float64), ld["rays"].astype(np.float64)
        cen64 = centres(ext64)
        for b, v in np.unique(np.stack([bb, ray_view[bb, cc]], 1), axis=0):
            if ok_a[b] and ray_can_win(ext64, cen64, rays64[b], ld["vis"][b], v, size, n_win[b], float(e_win[b]), delta):
                ok_a[b] = False
    mask_win = ld["inl"][ar, ld["best"]]
    tie = (ld["num"] == n_win[:, None]) & (np.abs(ld["emean"] - e_win[:, None]) <= delta) & ~undefined
    ok_b = ~(tie & (ld["inl"] != mask_win[:, None, :]).any(-1)).any(1)
    if point_bound is not None:
        X_win = ld["X"][ar, ld["best"]]
        far = ~(rel_point_distance(ld["X"], X_win[:, None, :], size) <= point_bound)
        ok_b &= ~((n_win >= 2)[:, None] & tie & far).any(1)
    return ok_a & ok_b


# --- cases --------------------------------------------------------------------------------------------------------------
def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def look_at(c, target):
    z = (target - c) / np.linalg.norm(target - c)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def cameras(R, c):
    return np.concatenate([R, -np.einsum("sij,sj->si", R, c)[:, :, None]], -1)


def observe(ext, X):
    y = np.einsum("sij,nj->sni", ext[:, :, :3], X) + ext[:, None, :, 3]
    with np.errstate(all="ignore"):
        return y[..., :2] / y[..., 2:], y[..., 2]


def random_visibility(rng, S, N, lo=2):
    vis = np.zeros((S, N))
    for n in range(N):
        vis[rng.permutation(S)[:rng.integers(lo, S + 1)], n] = 1.0
    return vis


def arc_cameras(rng, S, radius=6.0, span=90.0, jitter=0.3):
    a = np.deg2rad(np.linspace(-span / 2, span / 2, S))
    c = radius * np.stack([np.sin(a), 0.15 * rng.standard_normal(S), -np.cos(a)], 1) + jitter * rng.standard_normal((S, 3))
    R = np.stack([rodrigues(0.05 * rng.standard_normal(3)) @ look_at(c[s], 0.3 * rng.standard_normal(3)) for s in range(S)])
    return R, c


def finish(rng, R, c, X, noise, outliers, size, vis=None, scale=1.0, offset=0.0, vis_lo=2, per_track=False, **kw):
    """Observations of X (N,3) in the cameras (R, c), moved to scene units `scale` and `offset` scene sizes from the origin,
    plus noise and gross outliers (the draws do not depend on scale and offset)."""
    S, N = len(R), len(X)
    shift = offset * size * scale * np.array([0.6, 0.48, 0.64])
    ext = cameras(R, scale * c + shift)
    tn, _ = observe(ext, scale * X + shift)
    tn = tn + noise * rng.standard_normal(tn.shape)
    gross = rng.random((S, N)) < outliers
    if per_track:                                   # the same share of every track, so that no track is left with two good views
        gross = np.stack([rng.permutation(S) < round(outliers * S) for _ in range(N)], 1)
    tn = np.where(gross[:, :, None], rng.uniform(-0.6, 0.6, tn.shape), tn)
    vis = random_visibility(rng, S, N, vis_lo) if vis is None else vis
    return dict(ext=ext, tn=np.ascontiguousarray(tn), vis=vis, size=size * scale, **kw)


def arc_case(seed, S, N=96, noise=1e-3, outliers=0.05, span=90.0, iters=256, with_score=False, vis=None, **kw):
    rng = np.random.default_rng(seed)
    R, c = arc_cameras(rng, S, span=span)
    X = rng.uniform(-1, 1, (N, 3))
    case = finish(rng, R, c, X, noise, outliers, 6.0, vis=vis, iters=iters, **kw)
    if with_score:
        score = np.where(rng.random((S, N)) < 0.1, 0.4, 0.9)
        score[:, ::17] = 0.3
        case["score"] = score
    return case


def forward_case(seed, S=12, N=160):
    rng = np.random.default_rng(seed)
    c = np.stack([0.03 * rng.standard_normal(S), 0.03 * rng.standard_normal(S), np.linspace(-8, -4, S)], 1)
    R = np.stack([rodrigues(0.02 * rng.standard_normal(3)) for _ in range(S)])
    X = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.5, 1.5, N), rng.uniform(-1, 1, N)], 1)
    return finish(rng, R, c, X, 5e-4, 0.01, 8.0, iters=256)


def lowpar_case(seed, S=10, N=160):
    rng = np.random.default_rng(seed)
    c = np.stack([np.linspace(-0.16, 0.16, S), 0.02 * rng.standard_normal(S), np.full(S, -7.0)], 1)
    R = np.stack([rodrigues(0.03 * rng.standard_normal(3)) for _ in range(S)])
    return finish(rng, R, c, rng.uniform(-1, 1, (N, 3)), 2e-4, 0.01, 7.0, iters=256)


def dup_case(seed, S=13, N=160):
    """Every third camera at the centre of the one before it with another rotation; the last camera equals camera 0, and
    so do its observations of the even tracks."""
    rng = np.random.default_rng(seed)
    R, c = arc_cameras(rng, S)
    for s in range(2, S, 3):
        c[s] = c[s - 1]
        R[s] = rodrigues(0.2 * rng.standard_normal(3)) @ R[s - 1]
    R[S - 1], c[S - 1] = R[0], c[0]
    case = finish(rng, R, c, rng.uniform(-1, 1, (N, 3)), 1e-3, 0.01, 6.0, iters=256)
    case["tn"][S - 1, ::2] = case["tn"][0, ::2]
    return case


def wide_case(seed, S=10, N=160):
    rng = np.random.default_rng(seed)
    R, c = arc_cameras(rng, S, radius=3.0, span=140.0, jitter=0.2)
    R = np.stack([rodrigues(rng.uniform(-0.9, 0.9, 3) * [1, 1, 0.5]) @ R[s] for s in range(S)])
    X = rng.uniform(-1, 1, (N, 3))
    tn, z = observe(cameras(R, c), X)
    seen = (z > 0.3) & (np.abs(tn).max(-1) <= 3.2)
    case = finish(rng, R, c, X, 1e-3, 0.01, 3.0, vis=seen * random_visibility(rng, S, N), iters=256)
    case["tn"] = np.where(seen[:, :, None], case["tn"], 0.0)
    return case


def exact_case(S=9, N=64):
    """No noise, R = I or a quarter turn about z, centres and points dyadic with depths 4 and 8: every normalised
    coordinate is exact and the rays of a track meet in a point."""
    rng = np.random.default_rng(77)
    c = np.stack([np.linspace(-2, 2, S), 0.25 * (np.arange(S) % 3 - 1), np.zeros(S)], 1)
    R = np.stack([np.eye(3)] * S)
    R[2] = R[6] = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    X = np.stack([rng.integers(-8, 9, N) / 8, rng.integers(-8, 9, N) / 8, 4.0 * rng.integers(1, 3, N)], 1)
    ext = cameras(R, c)
    tn, _ = observe(ext, X)
    return dict(ext=ext, tn=np.ascontiguousarray(tn), vis=random_visibility(rng, S, N), size=8.0, iters=256)


def behind_case(seed, S=10, N=160):
    rng = np.random.default_rng(seed)
    R, c = arc_cameras(rng, S)
    X = rng.uniform(-1, 1, (N, 3))
    for n in range(0, N, 3):
        j = rng.integers(S)
        X[n] = c[j] + R[j].T @ np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), -rng.uniform(0.5, 2.0)])
    return finish(rng, R, c, X, 1e-3, 0.01, 6.0, iters=256)


VIS_COUNTS = (0, 1, 2, 5, 6, 7, 12, 13, 63, 64, 65, 66)


def viscount_case(seed, S=66, per=8):
    rng = np.random.default_rng(seed)
    N = per * len(VIS_COUNTS)
    vis = np.zeros((S, N))
    for b, k in enumerate(VIS_COUNTS):
        for n in range(b * per, (b + 1) * per):
            vis[rng.permutation(S)[:k], n] = 1.0
    return arc_case(seed + 1, S, N, outliers=0.03, vis=vis)


def grid_stride_case(seed=5, N=8192 + 300, every=False):
    """S = 4, three reference chunks, more tracks than the launch has workgroups.  Built from rng.random and the four basic
    operations alone, so that the inputs are the same bits everywhere and the fixture carries their sha256 only.
    `every`: full visibility, no outliers and noise of the order of the inlier threshold -- every hypothesis has an inlier, so
    each chunk has a threshold of its own below 2 pi (a well conditioned arc cosine close to MAX_RAD): the per-chunk maxima
    a workgroup flushes at a chunk change, and the re-launch with more than one chunk, are then visible in the output."""
    rng = np.random.default_rng(seed)
    c = np.array([[-1.5, 0, 0], [-0.5, 0.25, 0], [0.5, -0.25, 0], [1.5, 0, 0.5]])
    ext = cameras(np.stack([np.eye(3)] * 4), c)
    X = np.stack([2 * rng.random(N) - 1, 2 * rng.random(N) - 1, 4 + 2 * rng.random(N)], 1)
    d = X[None] - c[:, None]
    # (`every`: more noise on the tracks that share a workgroup with a track of the last chunk, so that the largest mean error
    #  of the first chunk is among them and above the last chunk's -- a maximum carried over or dropped at the change shows)
    amp = np.where(np.arange(N) < N - 8192, 3.6e-2, 3e-2)[None, :, None] if every else 2e-3
    tn = d[..., :2] / d[..., 2:] + amp * (rng.random((4, N, 2)) - 0.5)
    gross = rng.random((4, N)) < (0.0 if every else 0.03)
    tn = np.where(gross[:, :, None], rng.random((4, N, 2)) - 0.5, tn)
    vis = (rng.random((4, N)) > (-1.0 if every else 0.2)) * 1.0
    return dict(ext=ext, tn=np.ascontiguousarray(tn), vis=vis, size=6.0, iters=256, max_pts=12000, hashed=True)


def rethreshold_case(seed, S=6, N=64):
    """Full visibility, no outliers, wide baselines: every hypothesis of the chunk has an inlier, so the chunk threshold is
    the largest mean inlier error, not 2 pi.  The noise is large so that this error is a well conditioned arc cosine."""
    rng = np.random.default_rng(seed)
    R, c = arc_cameras(rng, S, span=120.0)
    return finish(rng, R, c, rng.uniform(-1, 1, (N, 3)), 8e-3, 0.0, 6.0, vis=np.ones((S, N)), iters=256)


def pair_sweep_case(seed=9, S=41, N=50):
    """Camera 0 = [I | 0]; camera s at a baseline giving a parallax from 30 degrees (s = 1) down to 1e-7 rad (s = S - 1),
    log-uniform; the first half of the matches without noise, the second with 1e-4."""
    rng = np.random.default_rng(seed)
    par = np.exp(np.linspace(np.log(np.deg2rad(30.0)), np.log(1e-7), S - 1))
    c = np.zeros((S, 3))
    R = np.stack([np.eye(3)] * S)
    for s in range(1, S):
        d = np.array([1.0, 0.3 * rng.standard_normal(), 0.1 * rng.standard_normal()])
        c[s] = 6.0 * par[s - 1] * d / np.linalg.norm(d)
        R[s] = rodrigues(0.05 * rng.standard_normal(3))
    X = np.stack([rng.uniform(-1, 1, N), rng.uniform(-1, 1, N), rng.uniform(4, 8, N)], 1)
    ext = cameras(R, c)
    tn, _ = observe(ext, X)
    tn[:, N // 2:] += 1e-4 * rng.standard_normal((S, N - N // 2, 2))
    return dict(ext=ext, tn=np.ascontiguousarray(tn), size=6.0)


# name -> builder.  The torch seed of a case (the randperm draws of its chunks) is its position in this table + 100.
CASES = {
    "arc": lambda: arc_case(201, 30),
    "forward": lambda: forward_case(202),
    "lowpar": lambda: lowpar_case(203),
    "dup": lambda: dup_case(204),
    "wide": lambda: wide_case(205),
    "outl50": lambda: arc_case(206, 30, N=160, outliers=0.5, vis_lo=12, per_track=True),
    "exact": exact_case,
    "behind": lambda: behind_case(208),
    "scaled_small": lambda: arc_case(209, 12, N=160, outliers=0.01, scale=1e-2),
    "scaled_large": lambda: arc_case(209, 12, N=160, outliers=0.01, scale=1e2),
    "offset10": lambda: arc_case(209, 12, N=160, outliers=0.01, offset=10.0),
    "offset100": lambda: arc_case(209, 12, N=160, outliers=0.01, offset=100.0),
    "s2": lambda: arc_case(212, 2),
    "s3": lambda: arc_case(213, 3, N=160, outliers=0.01),
    "s4": lambda: arc_case(214, 4, N=160, outliers=0.01),
    "s8": lambda: arc_case(215, 8, N=160, outliers=0.01),
    "s64": lambda: arc_case(216, 64, N=64),
    "s65": lambda: arc_case(217, 65, N=64),
    "s66": lambda: arc_case(218, 66, N=64),
    "s130": lambda: arc_case(219, 130, N=64),
    "viscount": lambda: viscount_case(220),
    "it63": lambda: arc_case(221, 30, N=64, iters=63),
    "it64": lambda: arc_case(221, 30, N=64, iters=64),
    "it65": lambda: arc_case(221, 30, N=64, iters=65),
    "it128": lambda: arc_case(221, 30, N=64, iters=128),
    "it129": lambda: arc_case(221, 30, N=64, iters=129),
    "score": lambda: arc_case(222, 30, with_score=True),
    "multichunk": lambda: arc_case(223, 24, N=100, max_pts=900),
    "grid_stride": grid_stride_case,
    "rethreshold": lambda: rethreshold_case(224),
    "grid_stride_every": lambda: grid_stride_case(6, every=True),
}
NAMES = tuple(CASES)
MULTI_CHUNK = ("multichunk", "grid_stride", "grid_stride_every")
RETHRESHOLD = ("rethreshold", "grid_stride_every")       # every hypothesis of every chunk has an inlier
PAIR_GROUPS = ("pair_sweep", "exact", "dup", "outl50", "scaled_small", "scaled_large", "offset10", "offset100")


def build(name):
    case = CASES[name]()
    case.setdefault("max_pts", 819200)
    case.setdefault("score", None)
    case["seed"] = 100 + NAMES.index(name)
    case["name"] = name
    return case


def pair_name(group):
    return group if group == "pair_sweep" else "pair_" + group


def pair_inputs(group):
    case = pair_sweep_case() if group == "pair_sweep" else build(group)
    return case["ext"], case["tn"], case["size"]


def input_digest(case):
    h = hashlib.sha256()
    for k in ("ext", "tn", "vis"):
        h.update(np.ascontiguousarray(case[k], dtype=np.float64).tobytes())
    return h.hexdigest()


def invalid_vis_conf(case):
    ivc = case["vis"] <= 0.05
    if case.get("score") is not None:
        ivc = ivc | (case["score"] <= 0.5)
    return ivc.T                                                                  # (N,S)


def chunking(S, N, max_pts):
    """(chunk size, number of chunks) of the reference's torch.chunk split of the track axis."""
    splits = -(-S * N // max_pts) if S * N > max_pts else 1
    size = -(-N // splits)
    return size, -(-N // size)


def all_pairs(S):
    i, j = np.triu_indices(S, 1)
    return np.stack([i, j], 1)


def draw_pairs(case):
    """The hypothesis pairs of every chunk, drawn as the reference draws them (one torch.randperm per chunk from the global
    CPU generator, seeded with the case's seed right before the call)."""
    import torch
    S, N = case["tn"].shape[:2]
    comb = all_pairs(S)
    _, chunks = chunking(S, N, case["max_pts"])
    torch.manual_seed(case["seed"])
    out = []
    for _ in range(chunks):
        out.append(comb if case["iters"] > len(comb) else comb[torch.randperm(len(comb))[:case["iters"]].numpy()])
    return out


def reference(case, pairs, tracks=None, delta=None, bound=None, thresholds=None):
    """Long-double reference of a case -> dict of float64 / bool / int arrays, as the fixtures record them.  With `tracks`
    (an index array) only those tracks: the chunk thresholds, delta and dev64 then cover them alone, so a caller that
    compares with the record of the whole case passes the recorded `delta`, point `bound` and `thresholds`."""
    S, N = case["tn"].shape[:2]
    size, chunks = chunking(S, N, case["max_pts"])
    ivc = invalid_vis_conf(case)
    tn = case["tn"].transpose(1, 0, 2)
    tracks = np.arange(N) if tracks is None else np.asarray(tracks)
    parts = []
    for ch in range(chunks):
        sel = tracks[(tracks // size) == ch]
        ld = solve_chunk(case["ext"], tn[sel], ivc[sel], pairs[ch], LD, thres=None if thresholds is None else thresholds[ch])
        f64 = solve_chunk(case["ext"], tn[sel], ivc[sel], pairs[ch], np.float64, follow=ld)
        lap = solve_chunk(case["ext"], tn[sel], ivc[sel], pairs[ch], np.float64, follow=ld, lapack=True)
        parts.append((sel, ld, f64, lap))
    dq = max([decision_dev64(ld, f64) for _, ld, f64, _ in parts] + [0.0])
    delta = max(DELTA_FLOOR, MARGIN * dq) if delta is None else float(delta)
    out = dict(points=np.zeros((len(tracks), 3)), num=np.zeros(len(tracks), np.int64), mask=np.zeros((len(tracks), S), bool),
               admitted=np.zeros(len(tracks), bool), thresholds=np.zeros(chunks), thresholds64=np.zeros(chunks),
               delta=delta, decision_dev64=dq)
    pos = {int(t): k for k, t in enumerate(tracks)}
    dev, dev_lapack = 0.0, 0.0
    for sel, ld, f64, lap in parts:
        ar = np.arange(len(sel))
        use = admit(ld, delta, None, case["size"]) & (ld["num"][ar, ld["best"]] >= 2)
        if use.any():
            dev = max(dev, float(rel_point_distance(f64["X"][ar, ld["best"]], ld["X"][ar, ld["best"]], case["size"])[use].max()))
            dev_lapack = max(dev_lapack,
                             float(rel_point_distance(lap["X"][ar, ld["best"]], ld["X"][ar, ld["best"]], case["size"])[use].max()))
    bound = max(POINT_FLOOR, MARGIN * dev) if bound is None else float(bound)
    for ch, (sel, ld, f64, _) in enumerate(parts):
        ar = np.arange(len(sel))
        k = np.array([pos[int(t)] for t in sel], dtype=np.int64)
        out["points"][k] = ld["X"][ar, ld["best"]].astype(np.float64)
        out["num"][k] = ld["num"][ar, ld["best"]]
        out["mask"][k] = ld["inl"][ar, ld["best"]]
        out["admitted"][k] = admit(ld, delta, bound, case["size"])
        out["thresholds"][ch], out["thresholds64"][ch] = float(ld["thres"]), float(f64["thres"])
    out["dev64"], out["dev64_lapack"], out["point_bound"] = dev, dev_lapack, bound
    return out


def pair_reference(ext, tn, dt=LD):
    """triangulate_by_pair in dtype dt: points (S-1,N,3), eigenvalues ascending (S-1,N,4), cheirality, angle (degrees)."""
    ext, tn = ext.astype(dt), tn.astype(dt)
    S, N = tn.shape[:2]
    rays = unit_rays(tn.transpose(1, 0, 2))
    M = view_matrices(ext, rays)                                                   # (N,S,4,4)
    A = (M[:, :1] + M[:, 1:]).transpose(1, 0, 2, 3)                                # (S-1,N,4,4)
    w, V = jacobi_eigh4(A.reshape(-1, 4, 4))
    with np.errstate(all="ignore"):
        X = (V[:, :3, 0] / V[:, 3:, 0]).reshape(S - 1, N, 3)
        cen = centres(ext)
        z0 = np.einsum("j,snj->sn", ext[0, 2, :3], X) + ext[0, 2, 3]
        zs = np.einsum("sj,snj->sn", ext[1:, 2, :3], X) + ext[1:, 2, 3][:, None]
        che = ~((z0 <= 0) | (zs <= 0))
        ang = tri_angle_deg(((X - cen[0]) ** 2).sum(-1), ((X - cen[1:, None]) ** 2).sum(-1),
                            ((cen[1:] - cen[0]) ** 2).sum(-1)[:, None])
    return dict(points=X, lam=w.reshape(S - 1, N, 4), che=che, ang=ang, A=A)


def direction_angle(X, X_ld):
    """Angle between the homogeneous directions (X, 1) and (X_ld, 1) (what the eigenvectors are, up to sign and scale)."""
    with np.errstate(all="ignore"):
        a = np.concatenate([X.astype(LD), np.ones(X.shape[:-1] + (1,), LD)], -1)
        b = np.concatenate([X_ld.astype(LD), np.ones(X_ld.shape[:-1] + (1,), LD)], -1)
        a = a / np.sqrt((a * a).sum(-1, keepdims=True))
        b = b / np.sqrt((b * b).sum(-1, keepdims=True))
        return (2 * np.arcsin(np.minimum(np.sqrt(((a - b) ** 2).sum(-1)) / 2, 1))).astype(np.float64)


def pair_condition(lam):
    """(relative gap (lambda_2 - lambda_1) / lambda_4, the angle unit EPS64 lambda_4 / (lambda_2 - lambda_1))."""
    with np.errstate(all="ignore"):
        gap = (lam[..., 1] - lam[..., 0]) / lam[..., 3]
        return gap, EPS64 / gap


def load(name):
    with np.load(os.path.join(GOLDEN, f"tri_regimes_{name}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def case_from_fixture(name, g=None):
    """The inputs of a case as the tests use them: recorded in the fixture, or rebuilt and checked against its digest."""
    g = load(name) if g is None else g
    if "tn" in g:
        case = dict(ext=g["ext"], tn=g["tn"], vis=g["vis"], score=g["score"] if "score" in g else None)
    else:
        case = build(name)
        assert input_digest(case) == str(g["digest"]), f"{name}: rebuilt inputs differ from the recorded digest"
    case.update(name=name, seed=int(g["seed"]), iters=int(g["iters"]), max_pts=int(g["max_pts"]), size=float(g["size"]))
    return case
