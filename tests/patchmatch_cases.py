"""Yardstick of the PatchMatch tests: a NumPy restatement of every entry of
vggsfm_amd/csrc/patchmatch/vggsfm_amd_patchmatch.h from the header's text, and the cases.  A helper, not a test.

Everything is float64 from the float32 pixels, vectorised over the pixels, with the header's operation order; the scene, the
shared arithmetic (relative_pose, transfer_project, bilinear) and the sweep that gives the starts are tests/mvs_cases.py's.
The window sums are taken one window pixel after the other in the header's order (``reverse=True``: in the reversed
order -- the spread between the two is what a change of summation order alone does).  The hash is restated in uint64."""
import functools
import math

import numpy as np

from tests import mvs_cases as C
from tests.mvs_cases import bilinear, inside_image, plane_sweep, relative_pose, scene, transfer_project

MAX_SOURCES, MAX_RADIUS = 8, 3
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-3, 0), (3, 0), (0, -3), (0, 3))      # (dx, dy), the header's order
INIT_ITERATION = 0xFFFFFFFFFFFFFFFF                                                       # the `iteration` of plane_init's draw


# --------------------------------------------------------------------------------------------------- the hash
def _u64(v):
    return np.asarray(v, dtype=np.uint64)


def mix(z):
    """the splitmix64 finaliser, in uint64 arithmetic"""
    z = _u64(z)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hash5(seed, iteration, colour, pixel, draw):
    with np.errstate(over="ignore"):
        h = mix(_u64(seed) + np.uint64(0x9E3779B97F4A7C15))
    for word in (iteration, colour, pixel, draw):
        h = mix(h ^ _u64(word))
    return h


def unit(h):
    return (_u64(h) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def signed(h):
    return (_u64(h) >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0


# --------------------------------------------------------------------------------------------------- the cost
def _ordered_sum(a, reverse):
    idx = range(a.shape[0] - 1, -1, -1) if reverse else range(a.shape[0])
    s = np.zeros(a.shape[1:])
    for k in idx:
        s = s + a[k]
    return s


class Context:
    """What the cost of a plane needs besides the plane: the reference windows of every pixel (flattened, row-major),
    centred once, their rays, and the relative poses."""

    def __init__(self, frames, poses, cams, rays, ref, sources, radius, min_views, min_variance, reverse=False):
        S, H, W = frames.shape
        R = radius
        self.frames, self.cams, self.sources, self.H, self.W = frames, cams, list(sources), H, W
        self.min_views, self.reverse = min_views, reverse
        self.n = float((2 * R + 1) ** 2)
        dy, dx = [o.reshape(-1) for o in np.mgrid[-R:R + 1, -R:R + 1]]
        yy = np.clip(np.arange(H)[None, :, None] + dy[:, None, None], 0, H - 1) + np.zeros((1, 1, W), np.int64)
        xx = np.clip(np.arange(W)[None, None, :] + dx[:, None, None], 0, W - 1) + np.zeros((1, H, 1), np.int64)
        A = frames[ref].astype(np.float64)[yy, xx].reshape(len(dy), H * W)
        self.u, self.v = rays[yy, xx, 0].reshape(len(dy), H * W), rays[yy, xx, 1].reshape(len(dy), H * W)
        self.mA = _ordered_sum(A, reverse) / self.n
        self.a = A - self.mA
        self.sa = _ordered_sum(self.a, reverse)
        self.taa = _ordered_sum(self.a * self.a, reverse) - self.sa * self.sa / self.n
        self.textured = self.taa / self.n >= min_variance
        self.rel = [relative_pose(poses[ref], poses[s]) for s in sources]
        self.u0, self.v0 = rays[..., 0].reshape(-1), rays[..., 1].reshape(-1)
        self.R_ref = poses[ref][:, :3]


def cost_at(ctx, idx, al, be, ga):
    """the cost of plane (al, be, ga)[i] at pixel idx[i] (flat indices)"""
    u, v, a = ctx.u[:, idx], ctx.v[:, idx], ctx.a[:, idx]
    mA, sa, taa, n = ctx.mA[idx], ctx.sa[idx], ctx.taa[idx], ctx.n
    with np.errstate(all="ignore"):
        wk = (al * u + be * v) + ga
        q = 1.0 / wk
        positive = (wk > 0.0).all(0)
        acc, valid = np.zeros(len(idx)), np.zeros(len(idx), np.int64)
        for m, s in enumerate(ctx.sources):
            xs, ys, zs = transfer_project(ctx.rel[m], ctx.cams[s], u * q, v * q, q)
            ok = positive & ((zs > 0.0) & inside_image(xs, ys, ctx.H, ctx.W)).all(0)
            b = bilinear(ctx.frames[s], xs, ys) - mA
            sb, sbb, sab = _ordered_sum(b, ctx.reverse), _ordered_sum(b * b, ctx.reverse), _ordered_sum(a * b, ctx.reverse)
            tbb, tab = sbb - sb * sb / n, sab - sa * sb / n
            den = np.sqrt(taa * tbb)
            zncc = np.where(den > 0.0, tab / den, 0.0)
            acc = np.where(ok, acc + (1.0 - zncc), acc)
            valid = valid + ok
        return np.where(ctx.textured[idx] & (valid >= ctx.min_views), acc / valid, np.inf)


def plane_cost(ctx, plane):
    """entry plane_cost: (H,W) float64"""
    p = plane.reshape(-1, 3)
    return cost_at(ctx, np.arange(ctx.H * ctx.W), p[:, 0], p[:, 1], p[:, 2]).reshape(ctx.H, ctx.W)


def legality(al, be, ga, u0, v0, w_far, w_near, cos_tilt):
    """-> legal, and the relative distances of the two tests from their thresholds (inf where NaN; the range test over the
    unequal comparisons: w_c equal to an end of the range is the same bits on both sides, see LEGALITY_MARGIN)"""
    with np.errstate(all="ignore"):
        wc = (al * u0 + be * v0) + ga
        lhs = wc * wc
        rhs = ((cos_tilt * cos_tilt) * ((al * al + be * be) + ga * ga)) * ((u0 * u0 + v0 * v0) + 1.0)
        legal = (w_far <= wc) & (wc <= w_near) & (lhs >= rhs)
        lo, hi = np.abs(wc - w_far), np.abs(wc - w_near)
        m_range = np.minimum(np.where(lo > 0.0, lo, np.inf), np.where(hi > 0.0, hi, np.inf)) / w_near   # unequal ones only
        m_tilt = np.abs(lhs - rhs) / np.maximum(lhs, rhs)
    return legal, np.where(np.isnan(m_range), np.inf, m_range), np.where(np.isfinite(m_tilt), m_tilt, np.inf)


# --------------------------------------------------------------------------------------------------- the entries
def plane_init(depth, normals, pose, rays, w_far, w_near, cos_tilt, seed):
    """entry plane_init -> plane (H,W,3) float64, and the legality margins of the normals' planes"""
    H, W = depth.shape
    z = depth.astype(np.float64).reshape(-1)
    u0, v0 = rays[..., 0].reshape(-1), rays[..., 1].reshape(-1)
    has = z > 0.0
    plane = np.zeros((H * W, 3))
    with np.errstate(all="ignore"):
        plane[:, 2] = np.where(has, 1.0 / z, 0.0)
    margins = {"init_range": np.inf, "init_tilt": np.inf}
    if normals is not None:
        N = normals.astype(np.float64).reshape(-1, 3)
        R = pose[:, :3]
        n = [(R[i, 0] * N[:, 0] + R[i, 1] * N[:, 1]) + R[i, 2] * N[:, 2] for i in range(3)]
        with np.errstate(all="ignore"):
            d = ((n[0] * u0 + n[1] * v0) + n[2]) * z
            p = [c / d for c in n]
        legal, m_range, m_tilt = legality(p[0], p[1], p[2], u0, v0, w_far, w_near, cos_tilt)
        given = has & ((N[:, 0] != 0.0) | (N[:, 1] != 0.0) | (N[:, 2] != 0.0))
        take = given & legal
        for i in range(3):
            plane[:, i] = np.where(take, p[i], plane[:, i])
        margins = {"init_range": float(m_range[given].min(initial=np.inf)), "init_tilt": float(m_tilt[given].min(initial=np.inf))}
    pixel = np.arange(H * W, dtype=np.uint64)
    drawn = w_far + unit(hash5(seed, INIT_ITERATION, 0, pixel, 0)) * (w_near - w_far)
    plane[:, 2] = np.where(has, plane[:, 2], drawn)
    return plane.reshape(H, W, 3), margins


def step(ctx, plane, cost, w_far, w_near, depth_step, slope_step, cos_tilt, seed, iteration, colour):
    """entry step -> new plane, new cost (the inputs are not modified) and the margins of its decisions: gap (candidate
    against incumbent cost over the legal, finite, unequal comparisons), range and tilt (the legality tests)."""
    H, W = ctx.H, ctx.W
    ys, xs = np.mgrid[0:H, 0:W]
    active = ((xs + ys) & 1) == colour
    idx = np.flatnonzero(active.reshape(-1))
    ay, ax = ys.reshape(-1)[idx], xs.reshape(-1)[idx]
    flat = plane.reshape(-1, 3)
    al, be, ga = flat[idx, 0].copy(), flat[idx, 1].copy(), flat[idx, 2].copy()
    best = cost.reshape(-1)[idx].copy()
    u0, v0 = ctx.u0[idx], ctx.v0[idx]
    scale = math.ldexp(1.0, -iteration)
    r = [signed(hash5(seed, iteration, colour, idx.astype(np.uint64), i)) for i in range(3)]
    fa, fb, dw = (r[0] * scale) * slope_step, (r[1] * scale) * slope_step, (r[2] * scale) * depth_step
    gap = m_range = m_tilt = np.inf
    for cand in range(11):
        if cand < 8:
            dx, dy = NEIGHBOURS[cand]
            nx, ny = ax + dx, ay + dy
            use = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
            q = np.clip(ny, 0, H - 1) * W + np.clip(nx, 0, W - 1)
            ca, cb, cg = flat[q, 0], flat[q, 1], flat[q, 2]
        else:
            use = np.ones(len(idx), bool)
            wc = (al * u0 + be * v0) + ga
            ca = al + fa * wc if cand != 9 else al
            cb = be + fb * wc if cand != 9 else be
            wn = wc + dw if cand != 10 else wc
            cg = wn - (ca * u0 + cb * v0)
        legal, mr, mt = legality(ca, cb, cg, u0, v0, w_far, w_near, cos_tilt)
        m_range, m_tilt = min(m_range, float(mr[use].min(initial=np.inf))), min(m_tilt, float(mt[use].min(initial=np.inf)))
        legal = legal & use
        if not legal.any():
            continue
        value = np.full(len(idx), np.inf)
        value[legal] = cost_at(ctx, idx[legal], ca[legal], cb[legal], cg[legal])
        with np.errstate(invalid="ignore"):
            compared = legal & np.isfinite(value) & np.isfinite(best) & (value != best)
            gap = min(gap, float(np.abs(value - best)[compared].min(initial=np.inf)))
            better = legal & (value < best)
        al, be, ga, best = np.where(better, ca, al), np.where(better, cb, be), np.where(better, cg, ga), np.where(better, value, best)
    new_plane, new_cost = flat.copy(), cost.reshape(-1).copy()
    new_plane[idx, 0], new_plane[idx, 1], new_plane[idx, 2], new_cost[idx] = al, be, ga, best
    return new_plane.reshape(H, W, 3), new_cost.reshape(H, W), {"gap": gap, "range": m_range, "tilt": m_tilt}


def outputs(plane, cost, pose, rays, min_conf):
    """entry outputs -> depth, conf (H,W) float32, normal (H,W,3) float32, and |conf - min_conf| over the finite costs"""
    al, be, ga = plane[..., 0], plane[..., 1], plane[..., 2]
    R = pose[:, :3]
    with np.errstate(all="ignore"):
        wc = (al * rays[..., 0] + be * rays[..., 1]) + ga
        found = np.isfinite(cost)
        conf = np.where(found, 1.0 - cost, 0.0)
        keep = found & (wc > 0.0) & ~(conf < min_conf)
        m = [-((R[0, i] * al + R[1, i] * be) + R[2, i] * ga) for i in range(3)]
        length = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        depth = np.where(keep, 1.0 / wc, 0.0).astype(np.float32)
        normal = np.stack([np.where(keep & (length > 0.0), c / length, 0.0) for c in m], -1).astype(np.float32)
    return depth, conf.astype(np.float32), normal, float(np.abs(conf - min_conf)[found].min(initial=np.inf))


def tilt_cos(max_tilt_deg):
    """cos_max_tilt as vggsfm_amd.patchmatch derives it"""
    return min(max(math.cos(math.radians(max_tilt_deg)), 0.0), 1.0)


def refine(case, reverse=False):
    """A whole refinement of a case of cases(): plane_init, plane_cost, 2 x iterations steps, the outputs of every state.
    -> dict: states [(plane, cost)] (the start, then after every half-iteration), outs [(depth, conf, normal)] likewise,
    margins (the smallest of every decision over the run) and the parameters the entries take."""
    ctx = Context(case["frames"], case["poses"], case["cams"], case["rays"], case["ref"], case["sources"], case["radius"],
                  case["min_views"], case["min_variance"], reverse)
    w_far, w_near = case["inv_depth_far"], case["inv_depth_near"]
    cos_tilt = tilt_cos(case["max_tilt_deg"])
    pose = case["poses"][case["ref"]]
    plane, margins = plane_init(case["init_depth"], case["init_normals"], pose, case["rays"], w_far, w_near, cos_tilt, case["seed"])
    cost = plane_cost(ctx, plane)
    margins.update(gap=np.inf, range=np.inf, tilt=np.inf, conf=np.inf)
    states, outs = [(plane, cost)], []

    def emit():
        d, c, n, m = outputs(states[-1][0], states[-1][1], pose, case["rays"], case["min_conf"])
        margins["conf"] = min(margins["conf"], m)
        outs.append((d, c, n))
    emit()
    for it in range(case["iterations"]):
        for colour in (0, 1):
            plane, cost, m = step(ctx, plane, cost, w_far, w_near, case["depth_step"], case["slope_step"], cos_tilt, case["seed"],
                                  it, colour)
            for k in ("gap", "range", "tilt"):
                margins[k] = min(margins[k], m[k])
            states.append((plane, cost))
            emit()
    for pair in states + outs:
        for arr in pair:
            arr.setflags(write=False)
    return {"states": states, "outs": outs, "margins": margins, "ctx": ctx}


# --------------------------------------------------------------------------------------------------- the cases
def _sweep_case(sc, ref, sources, **kw):
    return C._case(sc, ref, sources, **kw)


def _spec(sweep, start=None, normals=None, iterations=2, seed=0, max_tilt_deg=75.0, slope_step=0.5):
    """a refinement case from a sweep case: the start is the restated sweep's depth map unless one is given"""
    args = {k: v for k, v in sweep.items() if k not in ("depth_near", "depth_far")}
    if start is None:
        start = plane_sweep(**args)["depth"]
    D = sweep["num_planes"]
    step_w = 2.0 * (sweep["inv_depth_near"] - sweep["inv_depth_far"]) / (D - 1) if D > 1 else 2.0 * (sweep["inv_depth_near"] - sweep["inv_depth_far"])
    return dict(sweep, init_depth=start, init_normals=normals, iterations=iterations, seed=seed, max_tilt_deg=max_tilt_deg,
                slope_step=slope_step, depth_step=step_w)


@functools.lru_cache(maxsize=None)
def scenes():
    return {0.0: scene(k=0.0), 0.08: scene(k=0.08)}


@functools.lru_cache(maxsize=None)
def cases():
    """STEP cases: the smallest shapes at which the kernels can go wrong (tests/test_gpu_patchmatch.py compares every
    half-iteration); TRUTH cases: views 0, 1, 2 of the k = 0 and k = 0.08 scenes, four iterations from the sweep's result."""
    from tests import fusion_cases as F

    sweeps, _ = C.sweep_cases()
    out = {name: _spec(sweeps[name]) for name in ("k0_24x32", "k08_24x32", "k08_21x35", "r1", "r3", "M1_ref2", "M8", "min_views2",
                                                  "wide_baseline", "facing_away", "constant_reference")}
    base = sweeps["k08_24x32"]
    start = out["k08_24x32"]["init_depth"]
    holes = start.copy()
    holes[np.random.default_rng(3).random(holes.shape) < 0.15] = 0.0
    out["holes"] = _spec(base, start=holes, seed=5)
    # normals of the swept map by the fusion's rule (restated): noisy, so that under a tilt limit of 30 degrees some
    # of their planes are legal and some are not
    nrm = F.depth_normals(start[None], base["poses"][base["ref"]][None], base["rays"][None], np.zeros(1, np.int32))["normals"][0]
    out["normals"] = _spec(base, start=holes, normals=nrm, seed=9, max_tilt_deg=30.0)
    for k, sc in scenes().items():
        for ref in range(3):
            srcs = [s for s in range(3) if s != ref]
            out[f"truth_k{int(round(100 * k)):02d}_v{ref}"] = _spec(_sweep_case(sc, ref, srcs), iterations=4)
    return out


STEP_CASES = ("k0_24x32", "k08_24x32", "k08_21x35", "r1", "r3", "M1_ref2", "M8", "min_views2", "wide_baseline", "facing_away",
              "constant_reference", "holes", "normals")
TRUTH_CASES = tuple(f"truth_k{k}_v{v}" for k in ("00", "08") for v in range(3))


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restated refinement of a case -- computed once, never modified"""
    return refine(cases()[name])


@functools.lru_cache(maxsize=None)
def order_spread():
    """The largest difference of a finite cost, over the start and the end of every case, between the restatement summing
    each window in the header's order and reversed (as mvs_cases.sweep_order_spread measures the sweep's)."""
    worst = 0.0
    for name, case in cases().items():
        ref = reference(name)
        rev = Context(case["frames"], case["poses"], case["cams"], case["rays"], case["ref"], case["sources"], case["radius"],
                      case["min_views"], case["min_variance"], True)
        for plane, _ in (ref["states"][0], ref["states"][-1]):
            a, b = plane_cost(ref["ctx"], plane), plane_cost(rev, plane)
            assert np.array_equal(np.isfinite(a), np.isfinite(b)), name
            both = np.isfinite(a)
            worst = max(worst, float(np.abs(a[both] - b[both]).max(initial=0.0)))
    return worst


# --------------------------------------------------------------------------------------------------- against truth
def truth_of(name):
    k, v = name.split("_")[1:]
    return scenes()[int(k[1:]) / 100.0]["truth"][int(v[1:])]


def truth_errors(depth, truth, dw):
    """(median, 90th percentile) of |1 / depth - 1 / truth| in plane spacings over the pixels with depth, and their share"""
    return C.truth_errors({"depth": depth, "index": np.where(depth > 0, 0, -1), "dw": dw}, truth)


def normal_angles(normal, valid):
    """angles in degrees between the normals of the valid pixels and the true plane's normal facing the cameras"""
    towards = -C._plane()[3]
    return np.degrees(np.arccos(np.clip(normal[valid].astype(np.float64) @ towards, -1.0, 1.0)))


def sweep_errors(name):
    """what the parent computes on the same case: the restated sweep's errors against truth"""
    case = cases()[name]
    args = {k: case[k] for k in ("frames", "poses", "cams", "rays", "ref", "sources", "inv_depth_far", "inv_depth_near",
                                 "num_planes", "radius", "min_views", "min_variance", "min_conf")}
    out = plane_sweep(**args)
    return C.truth_errors(out, truth_of(name)), out["dw"]


# measured on the restatement (tests/test_patchmatch_host.py prints them): per TRUTH case the median
# and the 90th percentile of the inverse-depth error in plane spacings and the median angle of the normal to the true
# plane's, in degrees.  The CPU and the GPU tests assert 2 x these.
TRUTH_MEASURED = {
    "truth_k00_v0": (0.0970, 6.3366, 2.498), "truth_k00_v1": (0.1111, 0.3688, 2.996), "truth_k00_v2": (0.1332, 2.1976, 2.297),
    "truth_k08_v0": (0.0860, 6.2272, 2.490), "truth_k08_v1": (0.1043, 0.3636, 2.989), "truth_k08_v2": (0.1255, 2.3468, 2.297),
}
# legality is a handful of IEEE products and sums in a fixed order on both sides, so nothing can differ; a decision closer
# than this (relative) to its threshold is still counted as a tie.  An exact equality is between identical bits (the
# inverse of a start depth that IS the range's end) and is no comparison at all.
LEGALITY_MARGIN = 1e-12
