"""The yardstick of the projection, filter and undistortion kernels (csrc/geometry.hip) beyond the mild goldens: a table of
cases built for the places where these kernels can go wrong (the pair search, the 64-frame words and the four lanes of a
point in the filter, the thresholds, the iteration control of the undistortion, the grid strides) and the reference's
formulas restated once in ``np.longdouble``: projection with the four distortion models and ``nan_to_num``, the filter
(squared reprojection error, the value for points behind a camera, count >= 2, ``hard_max``, "an inlier pair with an angle
>= ``min_tri_angle`` exists", the detail mask), the normalisation, and the literal Newton iteration of the undistortion
(central differences, the extra identity on the diagonal, the pivoted 2x2 solve, the whole-tensor stopping rule, the count).
Written from the reference's text and include/vggsfm_amd.h; oracle/geometry.py is not imported.  float32 tracks enter as
the numbers the kernel reads, widened exactly.  Only pairs of inlier frames are evaluated, so S = 4096 costs nothing.

Every decision comes with a margin, and is *admitted* -- compared bit for bit -- when its margin exceeds ``MARGIN`` times
what float64 does to that quantity on that case (the same restatement evaluated in float64, its largest deviation from
long double over the decisions near their threshold: ``dev``, and ``delta = MARGIN * dev``):

  inlier bit    |err - thr^2| / thr^2                      dev over the elements with err within [thr^2 / 4, 4 thr^2]
  cz <= 0       |cz| / (|E20 X| + |E21 Y| + |E22 Z| + |E23|); a sum whose non-zero terms are none, or two exact products that
                cancel, is zero in every arithmetic and is admitted as it is
  triangle      |largest inlier-pair angle - min_tri_angle| (a point is undecided only if no pair is decidedly above and
                some pair is in the band)                   dev over the pairs within [min / 4, 4 min]
  hard_max      compares input numbers, no arithmetic: float64 does nothing to it, always admitted
  non-finite    NaN and +-inf have no margin: admitted where the float64 evaluation lands in the same class
  stop rule     |max step^2 - max_step_norm| / max_step_norm per iteration, dev over [norm / 4, 4 norm]
  pivot swap    ||j10| - |j00|| / max(|j00|, |j10|) per element and iteration, dev over the elements with a ratio in [1/2, 2]

A point's mask is admitted when all of its bits and its triangle decision are; an undistorted track when the iteration
count and all of its swap decisions are.  No case may leave out more than ``CAP`` of its decisions, and none of those it was
built for (tests/test_geometry_cases.py).  Values (pixels, camera coordinates, normalised tracks) are held to
``MARGIN * dev64 + VALUE_ULPS * eps`` relative to max(|value|, 1), dev64 being the largest such deviation of the float64
evaluation from long double on the case; where the trajectory is admitted the device is also held to the suite's
kernel-versus-oracle bound (rtol 1e-12, atol 1e-14) against the float64 evaluation.

tests/test_geometry_cases.py checks the restatement against the reference project's recorded results
(tests/golden/geom_regimes_*.npz, written by oracle/gen_golden_geometry_regimes.py) and against oracle/geometry.py, and that
every case hits what it was built for; tests/test_gpu_geometry_regimes.py compares the device with the restatement.

Measured float64-versus-long-double deviations per case, from the fixtures (dev64 of the values, relative to
max(|value|, 1); `stop` and `swap` are the dev of those decisions), next to what an MI355X gave and the bound it is held to.  A
measured value is never its own bound.
  filter cases         no values; the largest dev over all of them: err 1.1e-13 of thr^2, cz 3.1e-16 of its scale, angle 1.6e-12
                       degrees; every decision of every case is admitted, and the device differs in no bit
  project_k0           S  4 P      34  pixels 7.0e-15 (device 6.9e-15, bound 7.0e-13)  camera 2.8e-16 (device 3.3e-16, bound 2.9e-14)
  project_k1           S  4 P      34  pixels 6.8e-15 (device 6.8e-15, bound 6.8e-13)  camera 3.0e-16 (device 3.5e-16, bound 3.0e-14)
  project_k2           S  4 P      34  pixels 8.5e-15 (device 8.5e-15, bound 8.5e-13)  camera 3.0e-16 (device 2.8e-16, bound 3.1e-14)
  project_k4           S  4 P      34  pixels 1.2e-14 (device 1.2e-14, bound 1.2e-12)  camera 2.6e-16 (device 2.8e-16, bound 2.7e-14)
  project_stride       S  1 P 1048876  pixels 4.6e-14 (device 4.6e-14, bound 4.6e-12)  camera 2.9e-16 (device 3.5e-16, bound 2.9e-14)
  project_p1           S  2 P       1  pixels 1.6e-16 (device 2.2e-16, bound 1.7e-14)  camera 7.4e-17 (device 1.4e-16, bound 8.3e-15)
  count1               S  2 P      12    1 iterations  values 4.4e-17 (device 0.0e+00, bound 5.3e-15)  stop 0.0e+00  swap 0.0e+00
  count7               S  2 P      12    7 iterations  values 5.2e-16 (device 5.6e-16, bound 5.3e-14)  stop 4.2e-10  swap 0.0e+00
  count8               S  2 P      12    8 iterations  values 4.9e-16 (device 4.4e-16, bound 5.0e-14)  stop 2.2e-10  swap 0.0e+00
  count9               S  2 P      12    9 iterations  values 2.8e-12 (device 2.8e-12, bound 2.8e-10)  stop 2.7e-10  swap 0.0e+00
  count16              S  2 P      12   16 iterations  values 5.6e-16 (device 5.6e-16, bound 5.7e-14)  stop 6.6e-11  swap 0.0e+00
  count17              S  2 P      12   17 iterations  values 6.7e-16 (device 6.7e-16, bound 6.8e-14)  stop 1.3e-10  swap 0.0e+00
  maxit1               S  2 P      12    1 iterations  values 2.4e-12 (device 2.4e-12, bound 2.4e-10)  stop 0.0e+00  swap 0.0e+00
  maxit2               S  2 P      12    2 iterations  values 9.2e-13 (device 9.2e-13, bound 9.2e-11)  stop 0.0e+00  swap 0.0e+00
  maxit5               S  2 P      12    5 iterations  values 2.4e-13 (device 2.4e-13, bound 2.4e-11)  stop 0.0e+00  swap 0.0e+00
  maxit8               S  2 P      12    8 iterations  values 9.0e-14 (device 9.0e-14, bound 9.0e-12)  stop 0.0e+00  swap 0.0e+00
  maxit12              S  2 P      12   12 iterations  values 1.2e-14 (device 1.2e-14, bound 1.2e-12)  stop 0.0e+00  swap 0.0e+00
  nonfinite_undistort  S  2 P      12  100 iterations  values 1.9e-16 (device 2.2e-16, bound 2.0e-14)  stop 0.0e+00  swap 0.0e+00
  global_stop          S  3 P      12   16 iterations  values 4.3e-16 (device 4.4e-16, bound 4.4e-14)  stop 1.5e-10  swap 0.0e+00
  swap_it1             S  2 P      12    1 iterations  values 7.1e-11 (device 7.1e-11, bound 7.1e-09)  stop 0.0e+00  swap 5.2e-11
  swap_it2             S  2 P      12    2 iterations  values 1.1e-10 (device 1.1e-10, bound 1.1e-08)  stop 0.0e+00  swap 5.2e-11
  eps_step             S  2 P       6   22 iterations  values 2.9e-10 (device 2.9e-10, bound 2.9e-08)  stop 1.2e-04  swap 0.0e+00
  undistort_stride     S 64 P   16389   38 iterations  values 6.8e-16 (device 6.7e-16, bound 6.9e-14)  stop 1.3e-10  swap 0.0e+00
  normalise_stride     S  1 P  524365    0 iterations  values 1.1e-16 (device 1.1e-16, bound 1.2e-14)  stop 0.0e+00  swap 0.0e+00
"""
import hashlib
import os

import numpy as np

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

MARGIN = 100.0                 # factor of safety on every float64-versus-long-double deviation (= triangulation_cases.MARGIN)
VALUE_ULPS = 4                 # rounding of the recorded long double to float64 and of the last operations, in units of eps
CAP = 0.01                     # no case leaves out more than this share of its decisions
EPS64 = float(np.finfo(np.float64).eps)
DBL_MAX = float(np.finfo(np.float64).max)
ORACLE_RTOL, ORACLE_ATOL = 1e-12, 1e-14      # the suite's kernel-versus-oracle bound (test_undistortion_roundtrip_property)
MAX_FRAMES = 4096              # vgg_filter_points refuses more


def _w(x, dt):
    """The float32 / float64 numbers of x, widened exactly to dt."""
    return None if x is None else np.asarray(x).astype(np.float64).astype(dt)


# --- the reference's formulas in any dtype -----------------------------------------------------------------------------------
def _range(x):
    """float64's range on a long-double value: beyond +-DBL_MAX the reference's arithmetic has +-inf (and what follows from
    it: inf - inf and 0 * inf are NaN), so every intermediate result of the projection passes through here."""
    if x.dtype != LD:
        return x
    with np.errstate(all="ignore"):
        return np.where(np.abs(x) > DBL_MAX, np.sign(x) * np.inf, x)


def distort(ep, u, v):
    """apply_distortion: ep (S,k), u, v (S,P) -> distorted (u, v)."""
    k, r = ep.shape[1], _range
    with np.errstate(all="ignore"):
        u2, v2 = r(u * u), r(v * v)
        r2 = r(u2 + v2)
        if k == 1:
            radial = r(ep[:, 0:1] * r2)
            du, dv = r(u * radial), r(v * radial)
        elif k == 2:
            radial = r(r(ep[:, 0:1] * r2) + r(r(ep[:, 1:2] * r2) * r2))
            du, dv = r(u * radial), r(v * radial)
        elif k == 4:
            k1, k2, p1, p2 = (ep[:, i:i + 1] for i in range(4))
            uv = r(u * v)
            radial = r(r(k1 * r2) + r(r(k2 * r2) * r2))
            du = r(r(r(u * radial) + r(2 * p1 * uv)) + r(p2 * r(r2 + r(2 * u2))))
            dv = r(r(r(v * radial) + r(2 * p2 * uv)) + r(p1 * r(r2 + r(2 * v2))))
        else:
            raise ValueError("Unsupported number of distortion parameters")
        return r(u + du), r(v + dv)


def value_class(x):
    """0 finite, 1 NaN, 2 above DBL_MAX (+inf in float64), 3 below -DBL_MAX."""
    with np.errstate(all="ignore"):
        return np.where(np.isnan(x), 1, np.where(x > DBL_MAX, 2, np.where(x < -DBL_MAX, 3, 0))).astype(np.int8)


def nan_to_num(x):
    """torch.nan_to_num(x, nan=0) of a float64 tensor: NaN -> 0, beyond +-DBL_MAX -> +-DBL_MAX."""
    dt = x.dtype.type
    cls = value_class(x)
    return np.where(cls == 1, dt(0), np.where(cls == 2, dt(DBL_MAX), np.where(cls == 3, dt(-DBL_MAX), x))), cls


def project(pts, ext, K, extra, dt):
    """project_3D_points + img_from_cam -> pixels (S,P,2) after nan_to_num, camera coordinates (S,3,P), the class of every
    pixel element before nan_to_num (S,P,2).  K None: camera coordinates only."""
    pts, ext = _w(pts, dt), _w(ext, dt)
    X = pts.T
    with np.errstate(all="ignore"):
        r = _range
        pc = r(r(r(r(ext[:, :, 0:1] * X[0]) + r(ext[:, :, 1:2] * X[1])) + r(ext[:, :, 2:3] * X[2])) + ext[:, :, 3:4])
        if K is None:
            return None, pc, None
        u, v = r(pc[:, 0] / pc[:, 2]), r(pc[:, 1] / pc[:, 2])
        if extra is not None:
            u, v = distort(_w(extra, dt), u, v)
        K = _w(K, dt)
        x = r(r(r(K[:, 0, 0:1] * u) + r(K[:, 0, 1:2] * v)) + K[:, 0, 2:3])
        y = r(r(r(K[:, 1, 0:1] * u) + r(K[:, 1, 1:2] * v)) + K[:, 1, 2:3])
    px, cls = nan_to_num(np.stack([x, y], -1))
    return px, pc, cls


def centres(ext):
    return -np.einsum("sji,sj->si", ext[:, :, :3], ext[:, :, 3])


def _sqnorm(d):
    with np.errstate(all="ignore"):
        n = np.sqrt((d * d).sum(-1))                 # the reference squares a norm
        return n * n


def tri_angle_deg(r1, r2, b):
    dt = r1.dtype.type
    pi = np.arccos(dt(-1))
    with np.errstate(all="ignore"):
        den = 2 * np.sqrt(r1 * r2)
        nom = r1 + r2 - b
        bad = den <= dt(np.float64(1e-12))
        c = np.clip(np.where(bad, dt(1), nom) / np.where(bad, dt(1), den), -1, 1)
        th = np.abs(np.arccos(c))
        return np.minimum(th, pi - th) * (180 / pi)


def _filter(job, dt):
    kw = job["kw"]
    thr2 = dt(np.float64(kw["max_reproj_error"]) * np.float64(kw["max_reproj_error"]))
    behind_value, hard_max, min_tri = dt(np.float64(kw["behind_value"])), kw["hard_max"], dt(np.float64(kw["min_tri_angle"]))
    pts, ext = _w(job["pts"], dt), _w(job["ext"], dt)
    S, P = ext.shape[0], pts.shape[0]
    px, pc, _ = project(job["pts"], job["ext"], job["K"], job["extra"], dt)
    with np.errstate(all="ignore"):
        d = _range(px - _w(job["tracks"], dt))
        n = np.sqrt(_range(_range(d[..., 0] * d[..., 0]) + _range(d[..., 1] * d[..., 1])))
        err_front = _range(n * n)
        cz = pc[:, 2]
        terms = np.stack([ext[:, 2, 0:1] * pts[:, 0], ext[:, 2, 1:2] * pts[:, 1], ext[:, 2, 2:3] * pts[:, 2],
                          np.broadcast_to(ext[:, 2, 3:4], (S, P))], 0)
        behind = cz <= 0
        err = np.where(behind, behind_value, err_front)
        inl = err <= thr2
    valid = inl.sum(0) >= 2
    if hard_max > 0:
        with np.errstate(all="ignore"):
            valid = valid & (np.abs(np.asarray(job["pts"], np.float64)) <= hard_max).all(-1)
    cen = centres(ext)
    angles, best = [None] * P, np.full(P, -1, dtype=dt)
    tri = np.zeros(P, bool)
    if kw["check_triangle"]:
        for p in np.nonzero(valid)[0]:
            idx = np.nonzero(inl[:, p])[0]
            ca = cen[idx]
            r = _sqnorm(pts[p] - ca)
            a, b = np.triu_indices(len(idx), 1)
            ang = tri_angle_deg(r[a], r[b], _sqnorm(ca[a] - ca[b]))
            angles[p] = ang
            with np.errstate(all="ignore"):
                best[p] = np.fmax.reduce(ang) if np.isfinite(ang).any() else dt(-1)
                tri[p] = bool((ang >= min_tri).any())
    mask = tri & valid if kw["check_triangle"] else valid
    detail = inl & tri[None] if kw["check_triangle"] else inl
    return dict(err=err, err_front=err_front, cz=cz, terms=terms, behind=behind, inl=inl, valid=valid, angles=angles, best=best,
                tri=tri, mask=mask, detail=detail, thr2=thr2, min_tri=min_tri)


def _same_class(a, b):
    """Non-finite values of a (long double) against b (float64): both NaN, or both beyond DBL_MAX on the same side."""
    return value_class(a) == value_class(b.astype(LD))


def _dev(a, b, where, scale):
    """Largest |a - b| / scale over `where` and finite differences (0 if none)."""
    with np.errstate(all="ignore"):
        d = np.abs(a.astype(LD) - b.astype(LD)) / scale
    d = d[where & np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


def eval_filter(job):
    """Long-double result of a filter case, its admitted decisions and the figures behind them."""
    ld, f64 = _filter(job, LD), _filter(job, np.float64)
    kw = job["kw"]
    thr2, min_tri = ld["thr2"], ld["min_tri"]
    with np.errstate(all="ignore"):
        # cz <= 0
        scale = np.abs(ld["terms"]).sum(0)
        nz = ld["terms"] != 0
        exact_products = (ld["terms"] == f64["terms"].astype(LD)).all(0)
        exact_zero = (ld["cz"] == 0) & ((nz.sum(0) == 0) | ((nz.sum(0) == 2) & exact_products))
        fin_cz = np.isfinite(ld["cz"]) & (scale > 0) & np.isfinite(scale)
        dev_cz = _dev(ld["cz"], f64["cz"], fin_cz, np.where(fin_cz, scale, 1))
        adm_cz = np.where(np.isfinite(ld["cz"]), exact_zero | (fin_cz & (np.abs(ld["cz"]) / np.where(fin_cz, scale, 1) > MARGIN * dev_cz)),
                          _same_class(ld["cz"], f64["cz"]))
        # err <= thr^2
        e = ld["err_front"]
        band = np.isfinite(e) & (e >= thr2 / 4) & (e <= 4 * thr2) & ~ld["behind"]
        dev_err = _dev(e, f64["err_front"], band, thr2)
        adm_err = np.where(ld["behind"], True, np.where(np.isfinite(e), np.abs(e - thr2) / thr2 > MARGIN * dev_err,
                                                        _same_class(e, f64["err_front"])))
    adm_bit = adm_cz & adm_err
    # the triangle test
    P = len(ld["mask"])
    dev_ang = 0.0
    for p in range(P):
        a, b = ld["angles"][p], f64["angles"][p]
        if a is not None and b is not None and a.shape == b.shape and a.size:
            dev_ang = max(dev_ang, _dev(a, b, (a >= min_tri / 4) & (a <= 4 * min_tri), 1))
    with np.errstate(all="ignore"):
        adm_tri = ~ld["valid"] | (not kw["check_triangle"]) | (np.abs(ld["best"] - min_tri) > MARGIN * dev_ang)
    adm_mask = adm_bit.all(0) & adm_tri
    adm_detail = adm_bit & adm_mask[None] if kw["check_triangle"] else adm_bit & np.ones(P, bool)[None]
    return dict(mask=ld["mask"], detail=ld["detail"], inlier=ld["inl"], adm_mask=adm_mask, adm_detail=adm_detail,
                best=ld["best"].astype(np.float64), f64_mask=f64["mask"], f64_detail=f64["detail"],
                figures=np.array([dev_err, dev_cz, dev_ang]))


def eval_project(job):
    px, pc, cls = project(job["pts"], job["ext"], job["K"], job["extra"], LD)
    px64, pc64, cls64 = project(job["pts"], job["ext"], job["K"], job["extra"], np.float64)
    adm = cls == cls64                      # NaN and overflow have no margin: the class float64 itself lands in
    fin = adm & (cls == 0)
    dev_px = _dev(px, px64, fin, np.maximum(np.abs(px), 1))
    dev_pc = _dev(pc, pc64, np.isfinite(pc), np.maximum(np.abs(pc), 1))
    return dict(px=px.astype(np.float64), pc=pc.astype(np.float64), cls=cls, adm=adm, f64_px=px64, f64_pc=pc64,
                figures=np.array([dev_px, dev_pc]))


def normalise(tracks, K, dt):
    t, K = _w(tracks, dt), _w(K, dt)
    with np.errstate(all="ignore"):
        return (t[..., 0] - K[:, 0, 2:3]) / K[:, 0, 0:1], (t[..., 1] - K[:, 1, 2:3]) / K[:, 1, 1:2]


def _undistort(job, dt, follow=None):
    """cam_from_img: normalisation and, with extra parameters, iterative_undistortion step by step.  `follow` (the long-double
    run): take its swap decisions and its iteration count, so that every quantity has its counterpart."""
    u, v = normalise(job["tracks"], job["K"], dt)
    if job["extra"] is None:
        return dict(u=u, v=v, iters=0, maxsq=[], swap=[], j00=[], j10=[], u11=[])
    ep = _w(job["extra"], dt)
    eps, rel, msn = dt(EPS64), dt(np.float64(1e-6)), dt(np.float64(1e-10))
    ou, ov = u.copy(), v.copy()
    log = dict(maxsq=[], swap=[], j00=[], j10=[], u11=[])
    iters = 0
    with np.errstate(all="ignore"):
        for it in range(job["max_iterations"]):
            iters += 1
            ud, vd = distort(ep, u, v)
            dx, dy = ou - ud, ov - vd
            su, sv = np.maximum(np.abs(u) * rel, eps), np.maximum(np.abs(v) * rel, eps)
            pu, mu = distort(ep, u + su, v), distort(ep, u - su, v)
            pv, mv = distort(ep, u, v + sv), distort(ep, u, v - sv)
            j00, j01 = (pu[0] - mu[0]) / (2 * su) + 1, (pv[0] - mv[0]) / (2 * sv)
            j10, j11 = (pu[1] - mu[1]) / (2 * su), (pv[1] - mv[1]) / (2 * sv) + 1
            swap = (np.abs(j10) > np.abs(j00)) if follow is None else follow["swap"][it]
            a00, a01 = np.where(swap, j10, j00), np.where(swap, j11, j01)
            a10, a11 = np.where(swap, j00, j10), np.where(swap, j01, j11)
            b0, b1 = np.where(swap, dy, dx), np.where(swap, dx, dy)
            l10 = a10 / a00
            u11 = a11 - l10 * a01
            d1 = (b1 - l10 * b0) / u11
            d0 = (b0 - a01 * d1) / a00
            u, v = u + d0, v + d1
            sq = d0 * d0 + d1 * d1
            m = np.max(sq)                                            # torch.max: NaN if any
            for k, x in (("maxsq", m), ("swap", swap), ("j00", j00), ("j10", j10), ("u11", u11)):
                log[k].append(x)
            if (m < msn) if follow is None else (iters == follow["iters"]):
                break
    return dict(u=u, v=v, iters=iters, **log)


def eval_undistort(job):
    ld = _undistort(job, LD)
    f64 = _undistort(job, np.float64, follow=ld)
    free = _undistort(job, np.float64)
    msn = LD(np.float64(1e-10))
    shape = ld["u"].shape
    adm_count, dev_stop, dev_swap = True, 0.0, 0.0
    adm_elem = np.ones(shape, bool)
    swaps = np.zeros(max(ld["iters"], 1), np.int64)
    with np.errstate(all="ignore"):
        for m, m64 in zip(ld["maxsq"], f64["maxsq"]):
            if np.isfinite(m) and msn / 4 <= m <= 4 * msn:
                dev_stop = max(dev_stop, float(abs(m - LD(m64)) / msn))
        for it in range(ld["iters"]):
            hi = np.maximum(np.abs(ld["j00"][it]), np.abs(ld["j10"][it]))
            lo = np.minimum(np.abs(ld["j00"][it]), np.abs(ld["j10"][it]))
            near = np.isfinite(hi) & (2 * lo >= hi) & (hi > 0)
            q, q64 = np.abs(ld["j10"][it]) - np.abs(ld["j00"][it]), np.abs(f64["j10"][it]) - np.abs(f64["j00"][it])
            dev_swap = max(dev_swap, _dev(q, q64, near, np.where(near, hi, 1)))
        for it in range(ld["iters"]):
            m = ld["maxsq"][it]
            last = it == ld["iters"] - 1
            if np.isfinite(m):
                if not (last and it == job["max_iterations"] - 1 and not m < msn):     # (the cap ends the loop, no decision)
                    adm_count = adm_count and bool(abs(m - msn) / msn > MARGIN * dev_stop)
            else:
                adm_count = adm_count and (np.isnan(m) == np.isnan(f64["maxsq"][it]))
            hi = np.maximum(np.abs(ld["j00"][it]), np.abs(ld["j10"][it]))
            q = np.abs(np.abs(ld["j10"][it]) - np.abs(ld["j00"][it]))
            adm_elem &= np.where(np.isfinite(q) & (hi > 0), q / np.where(hi > 0, hi, 1) > MARGIN * dev_swap, True)
            swaps[it] = int((ld["swap"][it] & np.isfinite(q)).sum())
    val, val64 = np.stack([ld["u"], ld["v"]], -1), np.stack([f64["u"], f64["v"]], -1)
    fin = np.isfinite(val)
    adm_val = adm_elem[..., None] & fin & np.isfinite(val64)
    dev_val = _dev(val, val64, adm_val, np.maximum(np.abs(val), 1))
    u11_min = min([float(np.abs(u[s]).min()) for u, s in zip(ld["u11"], ld["swap"]) if s.any()] + [np.inf])
    return dict(values=val.astype(np.float64), iters=ld["iters"], adm_count=adm_count, adm_elem=adm_elem, swaps=swaps,
                f64_values=val64, f64_iters=free["iters"], f64_free_values=np.stack([free["u"], free["v"]], -1),
                maxsq=np.array([float(m) for m in ld["maxsq"]]), u11_min=u11_min, figures=np.array([dev_val, dev_stop, dev_swap]))


def evaluate(job):
    return dict(filter=eval_filter, project=eval_project, undistort=eval_undistort)[job["kind"]](job)


def value_bound(dev64):
    """Relative to max(|value|, 1)."""
    return MARGIN * float(dev64) + VALUE_ULPS * EPS64


def value_excess(got, ld, dev64, where):
    """Largest |got - ld| / max(|ld|, 1) over `where`, and the bound it is held to."""
    with np.errstate(all="ignore"):
        d = np.abs(got.astype(LD) - ld.astype(LD)) / np.maximum(np.abs(ld.astype(LD)), 1)
    d = np.where(np.isnan(d), np.inf, d)[where]
    return (float(d.max()) if d.size else 0.0), value_bound(dev64)


# --- builders: rng.random, the four operations and sqrt only, so that a seed gives the same bits everywhere ----------------
def quat_R(q):
    q = np.asarray(q, np.float64)
    w, x, y, z = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def small_R(rng, amp):
    return quat_R(np.concatenate([[1.0], amp * (2 * rng.random(3) - 1)]))


def cameras(R, c):
    R, c = np.asarray(R, np.float64), np.asarray(c, np.float64)
    return np.ascontiguousarray(np.concatenate([R, -np.einsum("sij,sj->si", R, c)[:, :, None]], -1))


FLIP = np.diag([-1.0, 1.0, -1.0])            # a camera looking along -z


def intrinsics(rng, S, skew=3.0, positive_skew=False):
    """fx != fy, skew present (projection uses it, cam_from_img ignores it), per frame."""
    K = np.zeros((S, 3, 3))
    K[:, 0, 0], K[:, 1, 1] = 1000 + 50 * rng.random(S), 900 + 50 * rng.random(S)
    K[:, 0, 1] = skew * (rng.random(S) if positive_skew else 2 * rng.random(S) - 1)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 512 + 10 * rng.random(S), 384 + 10 * rng.random(S), 1.0
    return K


def coefficients(rng, S, k, scale=1.0):
    """Per-frame distortion coefficients of the k-parameter model (None for k = 0)."""
    if k == 0:
        return None
    amp = np.array([0.1, 0.02, 0.005, 0.005])[:k]
    return scale * amp * (2 * rng.random((S, k)) - 1)


def unit2(rng, n):
    d = 2 * rng.random((n, 2)) - 1 + 1e-3
    return d / np.sqrt((d * d).sum(-1, keepdims=True))


def make_tracks(rng, job, offsets, f64, far=150.0):
    """tracks (S,P,2): the exact projection (float64 evaluation of the restatement) plus `far` pixels in a random direction,
    except where offsets[p] = {frame: length} places the track `length` pixels from the projection."""
    px, _, _ = project(job["pts"], job["ext"], job["K"], job["extra"], np.float64)
    S, P = px.shape[:2]
    tr = px + far * unit2(rng, S * P).reshape(S, P, 2)
    for p, d in enumerate(offsets):
        for s, length in d.items():
            tr[s, p] = px[s, p] + length * unit2(rng, 1)[0]
    tr = np.where(np.isfinite(tr) & (np.abs(tr) < 1e30), tr, 0.0)
    return np.ascontiguousarray(tr if f64 else tr.astype(np.float32))


def filter_job(pts, ext, K, extra, **kw):
    kw = dict(dict(max_reproj_error=4.0, min_tri_angle=1.5, check_triangle=True, hard_max=300.0, behind_value=1e6), **kw)
    return dict(kind="filter", pts=np.ascontiguousarray(pts, dtype=np.float64), ext=ext, K=K, extra=extra, kw=kw)


def pair_list(S):
    """The frame pairs of the single-pair cases: every lane combination (a mod 4, b mod 4) and the word boundaries."""
    if S <= 8:
        return [(a, b) for a in range(S) for b in range(a + 1, S)]
    out = [(i, 4 + j) for i in range(4) for j in range(4)]
    for a, b in ((0, 1), (0, S - 1), (S - 2, S - 1), (62, 63), (63, 64), (64, 65), (63, 128), (127, 128)):
        if 0 <= a < b < S and (a, b) not in out:
            out.append((a, b))
    return out


TAN_ABOVE, TAN_BELOW = 0.0262, 0.0044          # tan(theta / 2) at theta = 3.0 and 0.5 degrees


def point_over_pair(ca, cb, tan_half, axis=(0.0, 0.0, 1.0)):
    """The point over the middle of the baseline, in the direction `axis` made perpendicular to it, that sees the baseline
    under the angle theta."""
    base = cb - ca
    B = np.sqrt((base * base).sum())
    bh = base / B
    n = np.asarray(axis) - (np.asarray(axis) * bh).sum() * bh
    n = n / np.sqrt((n * n).sum())
    return (ca + cb) / 2 + B / (2 * tan_half) * n


def pair_case(seed, S, P, k, f64):
    """Each point is an inlier in exactly two frames; even points see that pair under 3 to 4 degrees, odd ones under 0.5
    to 1."""
    rng = np.random.default_rng(seed)
    c = (rng.random((S, 3)) - 0.5) * np.array([1.0, 1.0, 0.2])
    ext = cameras([small_R(rng, 0.03) for _ in range(S)], c)
    pairs = pair_list(S)
    chosen = np.array([pairs[(p // 2) % len(pairs)] for p in range(P)]).reshape(P, 2)
    above = np.arange(P) % 2 == 0
    pts = np.stack([point_over_pair(c[a], c[b], (TAN_ABOVE * (1 + 0.3 * rng.random())) if up else TAN_BELOW * (1 + rng.random()))
                    for (a, b), up in zip(chosen, above)])
    job = filter_job(pts, ext, intrinsics(rng, S), coefficients(rng, S, k))
    lengths = (0.0, 0.5, 2.0, 3.0)
    job["tracks"] = make_tracks(rng, job, [{a: lengths[p % 4], b: lengths[(p // 4) % 4]} for p, (a, b) in enumerate(chosen)], f64)
    job["expect"] = dict(pair=chosen, above=above)
    return job


def _looking_up(rng, c, amp=0.02):
    return cameras([small_R(rng, amp) for _ in range(len(c))], c)


def _all_inlier_job(rng, pts, ext, k=0, f64=False, **kw):
    S = len(ext)
    job = filter_job(pts, ext, intrinsics(rng, S), coefficients(rng, S, k), **kw)
    job["tracks"] = make_tracks(rng, job, [{s: 0.25 for s in range(S)} for _ in range(len(pts))], f64)
    return job


def loop_case():
    """A closed camera path (a square of side 1, 10 frames a side): the frames furthest apart in index are neighbours in
    space.  Points over the middle at growing distance: accepted through an inner pair, then rejected."""
    rng = np.random.default_rng(11)
    t = np.arange(10) / 10
    o, z = np.ones(10), np.zeros(10)
    c = np.concatenate([np.stack([t, z, z], 1), np.stack([o, t, z], 1), np.stack([1 - t, o, z], 1), np.stack([z, 1 - t, z], 1)])
    dist = np.array([10.0, 20.0, 30.0, 45.0, 70.0, 100.0])         # the diagonal sqrt(2) subtends 1.5 degrees at 54
    pts = np.stack([0.5 + 0 * dist, 0.5 + 0 * dist, dist], 1)
    job = _all_inlier_job(rng, pts, _looking_up(rng, c), k=1)
    job["expect"] = dict(mask=dist < 54, inliers=40)
    return job


def widest_case():
    """A tight cluster of cameras, frames 0 and S-1 moved out to x = -1 and +1: only the widest pair can qualify."""
    rng = np.random.default_rng(12)
    S = 30
    c = 0.01 * (rng.random((S, 3)) - 0.5)
    c[0], c[S - 1] = (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0)
    dist = np.array([45.0, 50.0, 60.0, 70.0, 90.0, 120.0])         # widest pair 1.5 degrees at 76.4, cluster-outlier at 38.2
    pts = np.stack([0 * dist, 0 * dist, dist], 1)
    job = _all_inlier_job(rng, pts, _looking_up(rng, c), k=2, f64=True)
    job["expect"] = dict(mask=dist < 76, inliers=S)
    return job


def full_search_case():
    """S = 200 frames on a short line, every frame an inlier, no pair above 0.3 degrees: the whole search, ending False."""
    rng = np.random.default_rng(13)
    S = 200
    c = np.stack([0.001 * np.arange(S), 0.01 * (rng.random(S) - 0.5), 0.01 * (rng.random(S) - 0.5)], 1)
    pts = np.array([[0.1, 0.0, 50.0], [0.0, 0.3, 60.0], [-0.2, 0.1, 80.0]])
    job = _all_inlier_job(rng, pts, _looking_up(rng, c), k=4)
    job["expect"] = dict(mask=np.zeros(3, bool), inliers=S)
    return job


def between_case():
    """Two cameras facing each other with the points between them: theta near 180 degrees, and min(theta, pi - theta)
    rejects the points close to the axis."""
    rng = np.random.default_rng(14)
    ext = cameras([np.eye(3), FLIP], [[0.0, 0.0, -1.0], [0.0, 0.0, 1.0]])
    off = np.array([0.002, 0.005, 0.01, 0.02, 0.05, 0.2])            # pi - theta = 2 atan(off): 1.5 degrees at 0.0131
    pts = np.stack([off, 0 * off, 0.1 * (rng.random(6) - 0.5)], 1)
    job = _all_inlier_job(rng, pts, ext)
    job["expect"] = dict(mask=off > 0.0131, inliers=2)
    return job


def centre_case():
    """Points exactly at the centre of camera 0 (R = I, so cz == 0 and the ray length is 0 exactly), max_reproj_error 1000 so
    that the frame counts as an inlier: with frames 1 and 2 inliers too the pair (1, 2) accepts the point, with frame 2 off by
    2000 px only pairs with the camera it sits in are left and the denominator branch gives the angle 0."""
    rng = np.random.default_rng(15)
    ext = cameras([np.eye(3), small_R(rng, 0.02), small_R(rng, 0.02)], [[0.25, -0.5, 2.0], [-1.0, 0.0, -20.0], [1.0, 0.0, -20.0]])
    pts = np.array([[0.25, -0.5, 2.0]] * 2)
    job = filter_job(pts, ext, intrinsics(rng, 3), None, max_reproj_error=1000.0)
    job["tracks"] = make_tracks(rng, job, [{1: 0.5, 2: 0.5}, {1: 0.5, 2: 2000.0}], False)
    job["expect"] = dict(mask=np.array([True, False]))
    return job


def _two_cameras(rng, z=-20.0):
    return cameras([small_R(rng, 0.02), small_R(rng, 0.02)], [[-1.0, 0.0, z], [1.0, 0.0, z]])


def threshold_case(thr, chk, f64):
    """Errors at 0.999 and 1.001 of max_reproj_error in frames 0 and 1 (and 2): float64 decides them, which pins <= and the
    squared threshold."""
    rng = np.random.default_rng(20 + int(thr))
    S, P = 3, 16
    ext = cameras([small_R(rng, 0.02) for _ in range(S)], [[-1.0, 0.0, -20.0], [1.0, 0.0, -20.0], [0.0, 1.0, -20.0]])
    pts = np.stack([rng.random(P) - 0.5, rng.random(P) - 0.5, rng.random(P)], 1)
    job = filter_job(pts, ext, intrinsics(rng, S), coefficients(rng, S, 1), max_reproj_error=float(thr), check_triangle=chk)
    lo, hi = 0.999 * thr, 1.001 * thr
    table = ({0: lo, 1: lo}, {0: lo, 1: hi}, {0: hi, 1: hi}, {0: hi, 1: lo, 2: lo})
    job["tracks"] = make_tracks(rng, job, [table[p % 4] for p in range(P)], f64)
    job["expect"] = dict(mask=np.array([p % 4 in (0, 3) for p in range(P)]))
    return job


def hard_max_case(hard_max):
    """Coordinates exactly at 300, one ulp beyond, and negative, on each axis; every point an exact inlier of both frames."""
    rng = np.random.default_rng(30)
    nxt = float(np.nextafter(300.0, np.inf))
    vals = (300.0, nxt, -300.0, -nxt, 299.0)
    pts = []
    for axis in range(3):
        for v in vals:
            p = [10.0, -20.0, 100.0]
            p[axis] = v
            pts.append(p)
    pts.append([1e4, 0.0, 1e4])
    pts = np.array(pts)
    job = filter_job(pts, _two_cameras(rng, z=-400.0), intrinsics(rng, 2), None, hard_max=hard_max, check_triangle=False)
    job["tracks"] = make_tracks(rng, job, [{0: 0.5, 1: 0.5}] * len(pts), True)
    job["expect"] = dict(mask=(np.abs(pts) <= 300.0).all(1) if hard_max > 0 else np.ones(len(pts), bool))
    return job


def cz_case():
    """Frame 0 sees every point; frame 1 has R = I and its centre at (0, 0, 1): cz = Z - 1 exactly.  cz slightly positive,
    exactly 0 (with cx = 0 too: 0 / 0; and with cx != 0: inf) and negative; the track of frame 1 is where the pixel lands if
    the test on cz is left out (the principal point for u = v = 0, the origin for NaN -> 0)."""
    rng = np.random.default_rng(31)
    ext = cameras([small_R(rng, 0.02), np.eye(3)], [[3.0, 0.0, -20.0], [0.0, 0.0, 1.0]])
    t = 2.0 ** -30
    pts = np.array([[0.0, 0.0, 1 + t], [0.0, 0.0, 1.0], [0.0, 0.0, 1 - t], [0.5, 0.0, 1.0], [2.0 ** -40, 0.0, 1 + t], [0.0, 0.0, 2.0],
                    [0.0, 0.0, 0.0]])
    K = intrinsics(rng, 2)
    job = filter_job(pts, ext, K, None, check_triangle=False)
    job["tracks"] = make_tracks(rng, job, [{0: 0.5, 1: 0.0}] * len(pts), True)
    job["tracks"][1, 1] = 0.0                                            # NaN -> 0 lands here
    job["tracks"][1, [2, 6]] = K[1, :2, 2]                               # u = v = 0 lands here
    job["expect"] = dict(mask=np.array([True, False, False, False, True, True, False]))
    return job


def behind_case():
    """max_reproj_error = 1000: the value 1e6 given to a point behind a camera is <= 1000^2, so that frame is an inlier, as in
    the reference.  Frames 0 and 1 look along +z from x = -1 and 1, frame 2 along +z from z = -50, frame 3 along -z."""
    rng = np.random.default_rng(32)
    ext = cameras([np.eye(3), np.eye(3), small_R(rng, 0.02), FLIP], [[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -50.0], [0.0, 1.0, 0.0]])
    pts = np.array([[0.0, 0.0, -60.0], [0.1, 0.0, -30.0], [0.0, 0.2, 30.0], [0.0, 0.0, -200.0], [0.3, 0.0, 10.0]])
    job = filter_job(pts, ext, intrinsics(rng, 4), None, max_reproj_error=1000.0)
    job["tracks"] = make_tracks(rng, job, [{}] * len(pts), False, far=2000.0)
    # behind frames 0, 1, 2 | 0, 1 | 3 alone | 0, 1, 2 but under 0.6 degrees | 3 alone
    job["expect"] = dict(mask=np.array([True, True, False, False, False]))
    return job


def s1_case(chk):
    rng = np.random.default_rng(40)
    pts = np.stack([rng.random(5) - 0.5, rng.random(5) - 0.5, rng.random(5)], 1)
    job = filter_job(pts, cameras([small_R(rng, 0.02)], [[0.0, 0.0, -20.0]]), intrinsics(rng, 1), coefficients(rng, 1, 2), check_triangle=chk)
    job["tracks"] = make_tracks(rng, job, [{0: 0.5}, {}, {0: 3.0}, {0: 5.0}, {0: 0.0}], False)
    job["expect"] = dict(mask=np.zeros(5, bool), inliers0=np.array([True, False, True, False, True]))
    return job


def s4096_case():
    """The largest frame count the entry takes.  Cameras on a line 1 mm apart; point 0 is an inlier at frames 0, 63, 64 and
    4095 (only pairs with the last or the first frame qualify), point 1 at 2047 and 2048 -- a pair across a word boundary
    -- from 3 cm away."""
    rng = np.random.default_rng(41)
    S = MAX_FRAMES
    c = np.stack([0.001 * np.arange(S), np.zeros(S), np.zeros(S)], 1)
    pts = np.array([[2.0475, 0.0, 146.0], [2.0475, 0.0, 0.03]])
    job = filter_job(pts, cameras([np.eye(3)] * S, c), intrinsics(rng, S), coefficients(rng, S, 1))
    job["tracks"] = make_tracks(rng, job, [{0: 0.5, 63: 1.0, 64: 2.0, 4095: 3.0}, {2047: 0.5, 2048: 1.0}], False)
    job["expect"] = dict(mask=np.array([True, True]))
    return job


NONFINITE = dict(points=((5, 0, np.nan), (70, 1, np.inf), (131, 2, -np.inf)), tracks=((9, 0, np.nan), (75, 1, np.inf), (140, 0, -np.inf)))


def nonfinite_case(f64):
    """NaN and +-inf in a point and in a track element (at an inlier frame of its point) of a single-pair case of four
    workgroups: those points are rejected, every other point keeps its bits."""
    job = pair_case(50, 6, 200, 1, f64)
    for p, axis, v in NONFINITE["points"]:
        job["pts"][p, axis] = v
    for p, which, v in NONFINITE["tracks"]:
        job["tracks"][job["expect"]["pair"][p, which], p, which] = v
    hit = sorted(p for p, _, _ in NONFINITE["points"] + NONFINITE["tracks"])
    above = job["expect"]["above"].copy()
    above[hit] = False
    job["expect"] = dict(pair=job["expect"]["pair"], above=above, hit=np.array(hit))
    return job


# --- projection ----------------------------------------------------------------------------------------------------------
def project_case(k):
    """Points in front of and behind the cameras; in frame 2 (R = I, centre (0, 0, 1), no skew) cz == 0 exactly: 0 / 0, +-inf,
    0 * inf -> NaN -> 0; in frames 2 and 3 (R = I, centre 0, skew > 0) coordinates of 1e306 and 1e120 whose pixel, or whose
    distortion, overflows to +-DBL_MAX."""
    rng = np.random.default_rng(60 + k)
    ext = cameras([small_R(rng, 0.3), small_R(rng, 0.3), np.eye(3), np.eye(3)],
                  [[-1.0, 0.0, -4.0], [1.0, 0.5, -4.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    pts = np.concatenate([4 * (rng.random((24, 3)) - 0.5) + [0, 0, 1.0],
                          [[0.0, 0.0, 1.0], [0.5, 0.0, 1.0], [-0.5, 0.25, 1.0], [0.5, 0.25, 1.0], [0.0, -0.25, 1.0],
                           [1e306, 0.0, 2.0], [-1e306, 0.0, 2.0], [1e120, 1e120, 1.0], [-1e120, -1e120, 1.0], [1e306, 1e306, 1.0]]])
    K = intrinsics(rng, 4, positive_skew=True)
    K[2, 0, 1] = 0.0
    return dict(kind="project", pts=pts, ext=ext, K=K, extra=coefficients(rng, 4, k))


PROJECT_STRIDE_P, NORMALISE_STRIDE_P, UNDISTORT_STRIDE_P = 4096 * 256 + 300, 2048 * 256 + 77, 16384 + 5
PERIOD = 257                                  # prime: a wrong stride shows in every element


def project_unique_case(P, k, S):
    """The distinct points of a grid-stride case: the device gets them tiled with period P (prime)."""
    rng = np.random.default_rng(70 + P)
    pts = 4 * (rng.random((P, 3)) - 0.5) + [0, 0, 6.0]
    ext = cameras([small_R(rng, 0.1) for _ in range(S)], 0.5 * (rng.random((S, 3)) - 0.5))
    return dict(kind="project", pts=pts, ext=ext, K=intrinsics(rng, S), extra=coefficients(rng, S, k))


# --- cam_from_img ----------------------------------------------------------------------------------------------------------
def undistort_job(uv, K, extra, f64, max_iterations=100):
    """Tracks that normalise to (about) uv (S,P,2)."""
    uv = np.asarray(uv, np.float64)
    tr = np.stack([K[:, 0, 2:3] + K[:, 0, 0:1] * uv[..., 0], K[:, 1, 2:3] + K[:, 1, 1:2] * uv[..., 1]], -1)
    return dict(kind="undistort", tracks=np.ascontiguousarray(tr if f64 else tr.astype(np.float32)), K=K,
                extra=None if extra is None else np.ascontiguousarray(extra, dtype=np.float64), max_iterations=max_iterations)


RAYS = np.array([[1.0, 0.0], [0.0, 1.0], [0.6, 0.8], [-0.8, 0.6], [-0.6, -0.8], [0.28, -0.96]])
BASE_COEFF = np.array([[-0.3, 0.08, 0.004, -0.003], [0.25, -0.05, -0.002, 0.005]])


def ring_uv(S, P, r_max=0.9):
    r = r_max * (1 + np.arange(P)) / P
    return np.stack([(r[:, None] * RAYS[(np.arange(P) + s) % len(RAYS)]) for s in range(S)])


def count_case(k, scale, f64, max_iterations=100):
    """Two frames, tracks on rings out to a radius of 0.9, the coefficients BASE_COEFF[:, :k] * scale: `scale` sets how many
    iterations the whole tensor needs."""
    rng = np.random.default_rng(80 + k)
    return undistort_job(ring_uv(2, 12), intrinsics(rng, 2), scale * BASE_COEFF[:, :k], f64, max_iterations)


# name -> (k, scale, float64 tracks); the scales were tuned on the CPU with this restatement for the count in the name
COUNT_CASES = {"count1": (1, 0.0, False), "count7": (1, 0.004, False), "count8": (2, 0.01, True), "count9": (4, 0.02, False),
               "count16": (1, 0.28, True), "count17": (2, 0.5, False)}
MAX_ITERATIONS = (1, 2, 5, 8, 12)


def nonfinite_undistort_case():
    """One NaN and one inf track among finite ones: the maximum is never below the norm, so 100 iterations."""
    job = count_case(2, COUNT_CASES["count9"][1], False)
    job["tracks"][0, 3, 0] = np.nan
    job["tracks"][1, 7, 1] = np.inf
    return job


def global_stop_case():
    """Three frames, strong distortion in frame 1 only: frames 0 and 2 converge early and are stepped until frame 1 is done."""
    rng = np.random.default_rng(85)
    extra = np.array([[1e-4], [COUNT_CASES["count16"][1] * BASE_COEFF[0, 0]], [-1e-4]])
    return undistort_job(ring_uv(3, 12), intrinsics(rng, 3), extra, False)


def swap_case(max_iterations):
    """k1 = -2: j00 = 2 + k1 (3 u^2 + v^2) vanishes on 3 u^2 + v^2 = 1 while j10 = 2 k1 u v does not, so the first step swaps
    the rows there; fx = fy = 1024 and a principal point of (512, 384) make the float64 tracks normalise exactly."""
    K = np.zeros((2, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = 1024.0
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 2.0, 512.0, 384.0, 1.0
    d = 2.0 ** -20
    on = [(0.5, 0.5), (0.5 + d, 0.5), (0.5 - d, 0.5), (0.5, 0.5 + d), (0.25, 0.90138781886599732), (-0.5, 0.5), (0.5, -0.5 + d),
          (0.55, 0.55)]
    off = [(0.1, 0.1), (0.3, -0.2), (0.0, 0.4), (0.45, 0.2)]
    uv = np.array([on + off, off + on])
    return undistort_job(uv, K, np.array([[-2.0], [-2.0]]), True, max_iterations)


SWAPS_STEP1 = 16


def eps_case():
    """Tracks at the principal point and on its row and column: u = 0 or v = 0, the step is eps."""
    rng = np.random.default_rng(86)
    K = intrinsics(rng, 2)
    K[:, 0, 2], K[:, 1, 2] = [512.0, 500.5], [384.0, 390.25]              # float32 numbers
    uv = np.array([[(0.0, 0.0), (0.0, 0.4), (0.4, 0.0), (0.0, -0.7), (-0.7, 0.0), (0.3, 0.3)]] * 2)
    return undistort_job(uv, K, 1.0 * BASE_COEFF[:, :4], False)


def undistort_unique_case(S, P, k, f64):
    rng = np.random.default_rng(90 + S)
    uv = 1.2 * (rng.random((S, P, 2)) - 0.5)
    return undistort_job(uv, intrinsics(rng, S), coefficients(rng, S, k, scale=2.0), f64)


def tile(x, P, axis=1):
    """x tiled along `axis` to length P (the grid-stride cases)."""
    return np.ascontiguousarray(np.take(x, np.arange(P) % x.shape[axis], axis=axis))


# --- the table ---------------------------------------------------------------------------------------------------------------
# single-pair cases: S, P, distortion parameters, float64 tracks
PAIR_SHAPES = ((2, 1, 0, False), (2, 64, 1, True), (3, 63, 2, False), (4, 65, 4, True), (5, 20, 0, True), (63, 63, 1, False),
               (64, 64, 2, True), (65, 65, 4, False), (127, 48, 0, False), (128, 70, 1, True), (129, 130, 2, False),
               (257, 65, 4, True))

CASES = {}
for _i, (_S, _P, _k, _f) in enumerate(PAIR_SHAPES):
    CASES[f"pairs_s{_S}_p{_P}"] = (lambda i=_i, S=_S, P=_P, k=_k, f=_f: pair_case(100 + i, S, P, k, f))
CASES.update({
    "loop": loop_case, "widest": widest_case, "full_search": full_search_case, "between": between_case, "centre": centre_case,
    "thr1_chk0": lambda: threshold_case(1, False, True), "thr1_chk1": lambda: threshold_case(1, True, True),
    "thr4_chk0": lambda: threshold_case(4, False, False), "thr4_chk1": lambda: threshold_case(4, True, False),
    "thr8_chk0": lambda: threshold_case(8, False, False), "thr8_chk1": lambda: threshold_case(8, True, True),
    "hard_max": lambda: hard_max_case(300.0), "hard_max0": lambda: hard_max_case(0.0), "cz": cz_case, "behind1000": behind_case,
    "s1_chk1": lambda: s1_case(True), "s1_chk0": lambda: s1_case(False), "s4096": s4096_case,
    "nonfinite_f32": lambda: nonfinite_case(False), "nonfinite_f64": lambda: nonfinite_case(True),
    "project_k0": lambda: project_case(0), "project_k1": lambda: project_case(1), "project_k2": lambda: project_case(2),
    "project_k4": lambda: project_case(4),
    "project_stride": lambda: project_unique_case(PERIOD, 1, 1), "project_p1": lambda: project_unique_case(1, 2, 2),
})
for _name, (_k, _scale, _f) in COUNT_CASES.items():
    CASES[_name] = (lambda k=_k, s=_scale, f=_f: count_case(k, s, f))
for _m in MAX_ITERATIONS:
    CASES[f"maxit{_m}"] = (lambda m=_m: count_case(*COUNT_CASES["count17"], max_iterations=m))
CASES.update({
    "nonfinite_undistort": nonfinite_undistort_case, "global_stop": global_stop_case,
    "swap_it1": lambda: swap_case(1), "swap_it2": lambda: swap_case(2), "eps_step": eps_case,
    "undistort_stride": lambda: undistort_unique_case(64, 13, 4, False),
    "normalise_stride": lambda: dict(undistort_unique_case(1, PERIOD, 1, True), extra=None),
})
NAMES = tuple(CASES)
FILTER_NAMES = tuple(n for n in NAMES if n.startswith(("pairs_", "loop", "widest", "full_", "between", "centre", "thr", "hard_", "cz",
                                                       "behind", "s1_", "s4096", "nonfinite_f")))
PROJECT_NAMES = tuple(n for n in NAMES if n.startswith("project_"))
UNDISTORT_NAMES = tuple(n for n in NAMES if n not in FILTER_NAMES + PROJECT_NAMES)
PAIR_NAMES = tuple(n for n in NAMES if n.startswith("pairs_"))
REFERENCE_CANNOT_RUN = ("s4096",)              # the reference builds the (S^2, P) angle tensor: recorded from the restatement alone
FAMILIES = {"pairs": PAIR_NAMES, "filter": tuple(n for n in FILTER_NAMES if n not in PAIR_NAMES), "project": PROJECT_NAMES,
            "undistort": UNDISTORT_NAMES}
INPUT_KEYS = ("pts", "tracks", "ext", "K", "extra")


def build(name):
    job = CASES[name]()
    job["name"] = name
    return job


def input_digest(job):
    h = hashlib.sha256()
    for k in INPUT_KEYS:
        if job.get(k) is not None:
            h.update(k.encode() + np.ascontiguousarray(job[k]).tobytes())
    return h.hexdigest()


def family_of(name):
    return next(f for f, names in FAMILIES.items() if name in names)


_loaded = {}


def load(name):
    """The recorded figures of a case: {field: array}."""
    fam = family_of(name)
    if fam not in _loaded:
        with np.load(os.path.join(GOLDEN, f"geom_regimes_{fam}.npz"), allow_pickle=False) as z:
            _loaded[fam] = {k: z[k] for k in z.files}
    pre = name + "__"
    return {k[len(pre):]: v for k, v in _loaded[fam].items() if k.startswith(pre)}


def case_from_fixture(name, g=None):
    """The inputs of a case, rebuilt and checked against the recorded digest."""
    g = load(name) if g is None else g
    job = build(name)
    assert input_digest(job) == str(g["digest"]), f"{name}: rebuilt inputs differ from the recorded digest"
    return job
