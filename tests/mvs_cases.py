"""Yardstick of the multi-view stereo tests: a NumPy restatement of vggm_plane_sweep and vggm_consistency_filter from the
text of vggsfm_amd/csrc/mvs/vggsfm_amd_mvs.h, the analytic scene the tests run on, and their cases.  A helper, not a test.

Everything is float64 from the float32 pixels, vectorised over the pixels, with the header's operation order; the window
sums are taken one window pixel after the other in the header's order (``reverse=True``: in the reversed order -- the spread
between the two is what a change of summation order alone does).

The scene: a plane slanted by 12 degrees carrying a smooth, non-periodic texture (a sum of Gaussian blobs of random place,
size and sign, sigma >= 2.2 px in every view, so no wavelength below 6 px carries weight), rendered into every camera by
ray-plane intersection; the same intersection gives the true depth.  Cameras are hand-placed on a line in front of the
plane and look at its centre."""
import functools

import numpy as np

MAX_SOURCES = 8


# --------------------------------------------------------------------------------------------------- shared arithmetic
def relative_pose(pa, pb):
    """[R|t] (3,4) of view b from view a, in the header's order"""
    T = np.empty((3, 4))
    for i in range(3):
        for j in range(3):
            T[i, j] = (pb[i, 0] * pa[j, 0] + pb[i, 1] * pa[j, 1]) + pb[i, 2] * pa[j, 2]
        T[i, 3] = pb[i, 3] - ((T[i, 0] * pa[0, 3] + T[i, 1] * pa[1, 3]) + T[i, 2] * pa[2, 3])
    return T


def transfer_project(T, cam, p0, p1, p2):
    """-> x, y, X[2] (x, y meaningless where X[2] <= 0)"""
    X0 = ((T[0, 0] * p0 + T[0, 1] * p1) + T[0, 2] * p2) + T[0, 3]
    X1 = ((T[1, 0] * p0 + T[1, 1] * p1) + T[1, 2] * p2) + T[1, 3]
    X2 = ((T[2, 0] * p0 + T[2, 1] * p1) + T[2, 2] * p2) + T[2, 3]
    with np.errstate(all="ignore"):
        iz = 1.0 / X2
        a, b = X0 * iz, X1 * iz
        d = 1.0 + cam[3] * (a * a + b * b)
        return cam[0] * (a * d) + cam[1], cam[0] * (b * d) + cam[2], X2


def inside_image(x, y, H, W):
    with np.errstate(invalid="ignore"):
        return (x >= 0.0) & (x <= W - 1.0) & (y >= 0.0) & (y <= H - 1.0)


def bilinear(img, x, y):
    """the header's bilinear sample; coordinates outside are clamped (their samples are not used)"""
    H, W = img.shape
    x = np.clip(np.nan_to_num(x, nan=0.0), 0.0, W - 1.0)
    y = np.clip(np.nan_to_num(y, nan=0.0), 0.0, H - 1.0)
    xf, yf = np.floor(x), np.floor(y)
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = x - xf, y - yf
    I = img.astype(np.float64)
    s = ((1.0 - fx) * (1.0 - fy)) * I[y0, x0] + (fx * (1.0 - fy)) * I[y0, x1]
    s = s + ((1.0 - fx) * fy) * I[y1, x0]
    return s + (fx * fy) * I[y1, x1]


def _ordered_sum(a, reverse):
    """sum over axis 0 one slice after the other, ascending (or descending)"""
    idx = range(a.shape[0] - 1, -1, -1) if reverse else range(a.shape[0])
    s = np.zeros(a.shape[1:])
    for k in idx:
        s = s + a[k]
    return s


# --------------------------------------------------------------------------------------------------- entry 2
def plane_sweep(frames, poses, cams, rays, ref, sources, inv_depth_far, inv_depth_near, num_planes, radius, min_views,
                min_variance, min_conf, reverse=False):
    """-> dict: depth, conf (float32), index (int32), cost (D,H,W) float64, and the margins of every decision:
    gap (two lowest costs of a pixel), conf (|conf - min_conf|), variance (relative), parabola (|e|), edge (projections
    from the image border and from the camera plane, where they decide)."""
    S, H, W = frames.shape
    M, D, R = len(sources), num_planes, radius
    n = float((2 * R + 1) ** 2)
    dy, dx = [o.reshape(-1) for o in np.mgrid[-R:R + 1, -R:R + 1]]
    yy = np.clip(np.arange(H)[None, :, None] + dy[:, None, None], 0, H - 1) + np.zeros((1, 1, W), np.int64)
    xx = np.clip(np.arange(W)[None, None, :] + dx[:, None, None], 0, W - 1) + np.zeros((1, H, 1), np.int64)
    A = frames[ref].astype(np.float64)[yy, xx]                           # (n, H, W)
    u, v = rays[yy, xx, 0], rays[yy, xx, 1]
    mA = _ordered_sum(A, reverse) / n
    a = A - mA
    sa, saa = _ordered_sum(a, reverse), _ordered_sum(a * a, reverse)
    taa = saa - sa * sa / n
    var = taa / n
    textured = var >= min_variance
    dw = (inv_depth_near - inv_depth_far) / float(D - 1) if D > 1 else 0.0
    rel = [relative_pose(poses[ref], poses[s]) for s in sources]
    cost = np.full((D, H, W), np.inf)
    edge = np.inf
    for j in range(D):
        q = 1.0 / (inv_depth_far + float(j) * dw)
        acc, valid = np.zeros((H, W)), np.zeros((H, W), np.int64)
        for m, s in enumerate(sources):
            xs, ys, zs = transfer_project(rel[m], cams[s], u * q, v * q, q)
            front = zs > 0.0
            ok = (front & inside_image(xs, ys, H, W)).all(0)
            with np.errstate(invalid="ignore"):
                border = np.minimum(np.minimum(np.abs(xs), np.abs(xs - (W - 1.0))), np.minimum(np.abs(ys), np.abs(ys - (H - 1.0))))
            edge = min(edge, np.abs(zs).min(), np.nanmin(np.where(front, border, np.inf)))
            b = bilinear(frames[s], xs, ys) - mA
            sb, sbb, sab = _ordered_sum(b, reverse), _ordered_sum(b * b, reverse), _ordered_sum(a * b, reverse)
            tbb, tab = sbb - sb * sb / n, sab - sa * sb / n
            with np.errstate(all="ignore"):
                den = np.sqrt(taa * tbb)
                zncc = np.where(den > 0.0, tab / den, 0.0)
            acc = np.where(ok, acc + (1.0 - zncc), acc)
            valid = valid + ok
        with np.errstate(all="ignore"):
            cost[j] = np.where(textured & (valid >= min_views), acc / valid, np.inf)
    # selection
    finite = np.isfinite(cost)
    masked = np.where(finite, cost, np.inf)
    best_j = masked.argmin(0)                                            # first of equal minima
    found = finite.any(0)
    c = np.take_along_axis(masked, best_j[None], 0)[0]
    conf = np.where(found, 1.0 - c, 0.0)
    w = inv_depth_far + best_j.astype(np.float64) * dw
    jm, jp = np.clip(best_j - 1, 0, D - 1), np.clip(best_j + 1, 0, D - 1)
    cm, cp = np.take_along_axis(cost, jm[None], 0)[0], np.take_along_axis(cost, jp[None], 0)[0]
    with np.errstate(all="ignore"):
        e = (cm - 2.0 * c) + cp
        interior = found & (best_j > 0) & (best_j < D - 1) & np.isfinite(cm) & np.isfinite(cp)
        refine = interior & (e > 0.0)
        w = np.where(refine, w + ((0.5 * (cm - cp)) / e) * dw, w)
        keep = found & ~(conf < min_conf)
        depth = np.where(keep, 1.0 / w, 0.0).astype(np.float32)
    index = np.where(keep, best_j, -1).astype(np.int32)
    # margins
    two = np.sort(masked, axis=0)[:2] if D > 1 else None
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(two[1]), two[1] - two[0], np.inf).min() if D > 1 else np.inf
    margins = {"gap": float(gap),
               "conf": float(np.abs(conf - min_conf)[found].min(initial=np.inf)),
               "variance": float((np.abs(var - min_variance) / min_variance).min()) if min_variance > 0 else np.inf,
               "parabola": float(np.abs(e[interior]).min(initial=np.inf)),
               "edge": float(edge)}
    return {"depth": depth, "conf": conf.astype(np.float32), "index": index, "cost": cost, "margins": margins,
            "inv_depth": np.where(keep, w, np.nan), "dw": dw}


# --------------------------------------------------------------------------------------------------- entry 3
def consistency_filter(depth, poses, cams, rays, ray_index, ref, sources, rel_depth_tol, reproj_tol, min_consistent):
    """-> dict: depth (float32), count (int32), margins: reproj, rel_depth (distance of the two tests from their
    tolerances), round (distance of xs + 0.5, ys + 0.5 from an integer, where the nearest pixel is taken)."""
    S, H, W = depth.shape
    z = depth[ref].astype(np.float64)
    has = z > 0.0
    ys0, xs0 = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = rays[ray_index[ref]]
    p0, p1 = ray[..., 0] * z, ray[..., 1] * z
    count = np.zeros((H, W), np.int64)
    m_reproj = m_rel = m_round = np.inf
    for s in sources:
        xs, ys, zc = transfer_project(relative_pose(poses[ref], poses[s]), cams[s], p0, p1, z)
        with np.errstate(invalid="ignore"):
            xi, yi = np.floor(xs + 0.5), np.floor(ys + 0.5)
            go = has & (zc > 0.0) & inside_image(xi, yi, H, W)
        xq, yq = np.where(go, xi, 0).astype(np.int64), np.where(go, yi, 0).astype(np.int64)
        zs = depth[s].astype(np.float64)[yq, xq]
        front = has & (zc > 0.0)
        if front.any():
            fr = np.stack([xs[front] + 0.5, ys[front] + 0.5])
            m_round = min(m_round, float(np.abs(fr - np.round(fr)).min()))
        go = go & (zs > 0.0)
        rs = rays[ray_index[s]][yq, xq]
        xb, yb, zb = transfer_project(relative_pose(poses[s], poses[ref]), cams[ref], rs[..., 0] * zs, rs[..., 1] * zs, zs)
        go = go & (zb > 0.0)
        with np.errstate(all="ignore"):
            ex, ey = xb - xs0, yb - ys0
            dist = np.sqrt(ex * ex + ey * ey)
            relz = np.abs(zb - z) / z
            near = go & (dist <= reproj_tol) & (relz <= rel_depth_tol)
        if go.any():
            m_reproj = min(m_reproj, float(np.abs(dist[go] - reproj_tol).min()))
            m_rel = min(m_rel, float(np.abs(relz[go] - rel_depth_tol).min()))
        count = count + near
    out = np.where(count >= min_consistent, depth[ref], np.float32(0)).astype(np.float32)
    return {"depth": out, "count": count.astype(np.int32),
            "margins": {"reproj": m_reproj, "rel_depth": m_rel, "round": m_round}}


# --------------------------------------------------------------------------------------------------- the analytic scene
def pixel_rays(cam, H, W):
    """(H,W,2) undistorted normalised coordinates of the pixel centres (Newton on the radius, to machine precision)"""
    f, cx, cy, k = (float(c) for c in cam)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    xd, yd = (x - cx) / f, (y - cy) / f
    if k == 0.0:
        return np.stack([xd, yd], -1)
    rd = np.hypot(xd, yd)
    ru = rd.copy()
    for _ in range(60):
        ru = ru - (ru * (1.0 + k * ru * ru) - rd) / (1.0 + 3.0 * k * ru * ru)
    scale = np.where(rd > 0, ru / np.where(rd > 0, rd, 1.0), 1.0)
    return np.stack([xd * scale, yd * scale], -1)


def look_at(centre, target):
    z = (target - centre) / np.linalg.norm(target - centre)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return np.concatenate([R, (-R @ centre)[:, None]], 1)


PLANE_DEPTH, SLANT_DEG = 4.0, 12.0


def _plane():
    a = np.radians(SLANT_DEG)
    e1, e2 = np.array([np.cos(a), 0.0, np.sin(a)]), np.array([0.0, 1.0, 0.0])
    return np.array([0.0, 0.0, PLANE_DEPTH]), e1, e2, np.cross(e1, e2)


@functools.lru_cache(maxsize=None)
def _blobs(seed=7, count=900, half=6.0):
    g = np.random.default_rng(seed)
    return g.uniform(-half, half, (count, 2)), g.uniform(0.3, 0.6, count), g.uniform(0.4, 1.0, count) * g.choice([-1.0, 1.0], count)


def texture(s, t):
    """smooth, non-periodic: 0.5 + 0.18 x the sum of 900 signed Gaussian blobs (sigma 0.3 .. 0.6 plane units)"""
    pos, sig, amp = _blobs()
    out = np.zeros(s.shape)
    for (bs, bt), sg, am in zip(pos, sig, amp):
        out += am * np.exp(-((s - bs) ** 2 + (t - bt) ** 2) / (2.0 * sg * sg))
    return 0.5 + 0.18 * out


def render(pose, cam, H, W):
    """-> image (H,W) float32 and depth (H,W) float64 of the plane seen by one camera"""
    p0, e1, e2, nrm = _plane()
    rays = pixel_rays(cam, H, W)
    R, t = pose[:, :3], pose[:, 3]
    c = -R.T @ t
    d = np.concatenate([rays, np.ones((H, W, 1))], -1) @ R                   # R^T (u, v, 1) per pixel
    s = (nrm @ (p0 - c)) / (d @ nrm)                                         # camera-frame z of the intersection
    X = c + s[..., None] * d
    return texture((X - p0) @ e1, (X - p0) @ e2).astype(np.float32), s


def scene(H=24, W=32, xs=(-0.7, 0.0, 0.7), k=0.0, focal=None):
    """cameras at (x, 0.1 x, 0) looking at the plane's centre, focal 1.25 W by default -> dict of frames (S,H,W) float32,
    truth (S,H,W), poses (S,3,4), cams (S,4), rays (1,H,W,2), ray_index (S,)"""
    f = 1.25 * W if focal is None else focal
    cam = np.array([f, (W - 1) / 2.0 + 0.3, (H - 1) / 2.0 - 0.2, k])
    poses = np.stack([look_at(np.array([x, 0.1 * x, 0.0]), np.array([0.0, 0.0, PLANE_DEPTH])) for x in xs])
    cams = np.tile(cam, (len(xs), 1))
    out = [render(p, cam, H, W) for p in poses]
    return {"frames": np.stack([o[0] for o in out]), "truth": np.stack([o[1] for o in out]), "poses": poses, "cams": cams,
            "rays": pixel_rays(cam, H, W)[None], "ray_index": np.zeros(len(xs), np.int32)}


NEAR, FAR = 3.2, 5.0          # the plane's depth over every view of every scene here lies inside


# --------------------------------------------------------------------------------------------------- sweep cases
def _case(sc, ref, sources, D=24, radius=2, min_views=1, min_variance=1e-5, min_conf=0.5, near=NEAR, far=FAR):
    return dict(frames=sc["frames"], poses=sc["poses"], cams=sc["cams"], rays=sc["rays"][sc["ray_index"][ref]], ref=ref,
                sources=list(sources), inv_depth_far=1.0 / far, inv_depth_near=1.0 / near, num_planes=D, radius=radius,
                min_views=min_views, min_variance=min_variance, min_conf=min_conf, depth_near=near, depth_far=far)


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """The smallest shapes at which the sweep can go wrong (tests/test_gpu_mvs.py); `truth`: the cases with analytic truth."""
    a, b = scene(k=0.0), scene(k=0.08)
    odd = scene(H=21, W=35, k=0.08)
    nine = scene(xs=(-0.8, -0.6, -0.4, -0.2, 0.0, 0.2, 0.4, 0.6, 0.8))
    wide = scene(xs=(-0.7, 0.0, 0.7, 2.4))
    away = scene()
    away["poses"] = away["poses"].copy()
    away["poses"][2] = np.diag([-1.0, 1.0, -1.0]) @ away["poses"][2]        # turned by 180 degrees about its y axis
    const = scene()
    const["frames"] = const["frames"].copy()
    const["frames"][1] = 0.37
    cases = {
        "k0_24x32": _case(a, 1, (0, 2)), "k08_24x32": _case(b, 1, (0, 2)), "k08_21x35": _case(odd, 1, (2, 0)),
        "r1": _case(b, 1, (0, 2), radius=1), "r3": _case(b, 1, (0, 2), radius=3),
        "D1": _case(a, 1, (0, 2), D=1, near=3.9, far=4.1), "D2": _case(a, 1, (0, 2), D=2), "D3": _case(a, 1, (0, 2), D=3),
        "M1_ref2": _case(a, 2, (1,)), "M8": _case(nine, 4, (0, 1, 2, 3, 5, 6, 7, 8), min_views=2),
        "min_views2": _case(b, 1, (0, 2), min_views=2), "wide_baseline": _case(wide, 1, (0, 3, 2), min_views=2),
        "facing_away": _case(away, 1, (2,), min_views=1), "constant_reference": _case(const, 1, (0, 2)),
    }
    truth = {"k0_24x32": a["truth"][1], "k08_24x32": b["truth"][1]}
    return cases, truth


@functools.lru_cache(maxsize=None)
def sweep_reference(name, reverse=False):
    """the restatement of a case of sweep_cases() -- computed once, never modified"""
    case = {k: v for k, v in sweep_cases()[0][name].items() if k not in ("depth_near", "depth_far")}
    out = plane_sweep(**case, reverse=reverse)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sweep_order_spread():
    """The largest difference of a finite cost, over all cases, between the restatement summing each window in the
    header's order and reversed.  The GPU tolerance of the cost volume is 100 x this."""
    worst = 0.0
    for name in sweep_cases()[0]:
        a, b = sweep_reference(name)["cost"], sweep_reference(name, True)["cost"]
        assert np.array_equal(np.isfinite(a), np.isfinite(b)), name
        both = np.isfinite(a)
        worst = max(worst, float(np.abs(a[both] - b[both]).max(initial=0.0)))
    return worst


def truth_errors(out, truth):
    """(median, 90th percentile) of |1 / depth - 1 / truth| in plane spacings over the valid pixels, and their share"""
    valid = out["index"] >= 0
    err = np.abs(1.0 / out["depth"][valid].astype(np.float64) - 1.0 / truth[valid]) / out["dw"]
    return float(np.median(err)), float(np.percentile(err, 90)), float(valid.mean())


# measured on the restatement at 24 x 32, 3 views, 24 planes, radius 2 (tests/test_mvs_host.py prints them; DESIGN.md
# section 28), the worse of k = 0 and k = 0.08: median and 90th percentile of the inverse-depth error in plane spacings,
# and the share of pixels WITHOUT a depth (none).  The CPU and the GPU tests assert 2 x these.
TRUTH_MEDIAN, TRUTH_P90, TRUTH_INVALID = 0.3324, 1.0457, 0.0


# --------------------------------------------------------------------------------------------------- filter cases
@functools.lru_cache(maxsize=None)
def filter_cases():
    """Depth maps = the truth of the k = 0.08 scene (shared ray map), with holes, with a source that disagrees, and
    min_consistent 1 and 2; tolerances 1 % and 1 px."""
    sc = scene(k=0.08)
    g = np.random.default_rng(3)
    holes = sc["truth"].astype(np.float32)
    holes[g.random(holes.shape) < 0.15] = 0.0
    wrong = holes.copy()
    wrong[2] = np.where(wrong[2] > 0, wrong[2] * np.float32(1.06), 0).astype(np.float32)     # source 2 is 6 % off
    two = dict(sc, rays=np.concatenate([sc["rays"], sc["rays"]]), ray_index=np.array([1, 0, 1], np.int32))
    mk = lambda s, d, ref, src, mc: dict(depth=d, poses=s["poses"], cams=s["cams"], rays=s["rays"], ray_index=s["ray_index"],
                                         ref=ref, sources=list(src), rel_depth_tol=0.01, reproj_tol=1.0, min_consistent=mc)
    return {"holes_mc2": mk(sc, holes, 1, (0, 2), 2), "holes_mc1": mk(sc, holes, 1, (0, 2), 1),
            "disagree_mc2": mk(sc, wrong, 1, (0, 2), 2), "disagree_mc1": mk(sc, wrong, 0, (2, 1), 1),
            "two_ray_maps": mk(two, holes, 1, (2, 0), 2)}


@functools.lru_cache(maxsize=None)
def filter_reference(name):
    out = consistency_filter(**filter_cases()[name])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# --------------------------------------------------------------------------------------------------- reconstruction scene
def project(pose, cam, X):
    """pixels (P,2) and camera-frame z (P,) of world points X (P,3)"""
    Xc = X @ pose[:, :3].T + pose[:, 3]
    a, b = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    d = 1.0 + cam[3] * (a * a + b * b)
    return np.stack([cam[0] * (a * d) + cam[1], cam[0] * (b * d) + cam[2]], -1), Xc[:, 2]


@functools.lru_cache(maxsize=None)
def reconstruction_scene(count=400, seed=5):
    """6 frames of 48 x 64 under one SIMPLE_RADIAL camera (k = 0.08) on a line of 2.5 units, and `count` sparse points on
    the plane with their exact projections: what tests/test_gpu_mvs_reconstruct.py builds its reconstruction from."""
    sc = scene(H=48, W=64, xs=(-1.25, -0.75, -0.25, 0.25, 0.75, 1.25), k=0.08)
    p0, e1, e2, _ = _plane()
    st = np.random.default_rng(seed).uniform(-2.2, 2.2, (count, 2))
    X = p0 + st[:, :1] * e1 + st[:, 1:] * e2
    uv = np.stack([project(p, c, X)[0] for p, c in zip(sc["poses"], sc["cams"])])
    sc["points3D"], sc["tracks"] = X, uv
    sc["masks"] = inside_image(uv[..., 0], uv[..., 1], 48, 64)
    return sc
