"""Yardstick of the depth-map fusion tests: a NumPy restatement of vggf_depth_normals and vggf_fuse_view from the text of
vggsfm_amd/csrc/fuse/vggsfm_amd_fuse.h, the cases and their cached references.  A helper, not a test.

Everything is float64 from the float32 inputs, vectorised over the pixels of a view, with the header's operation order.  The
scene is the analytic one of tests/mvs_cases.py (a slanted, textured plane seen from a line of cameras); the depth maps are
its true depths rounded to float32, so a fused point lies on the plane up to that rounding and every normal is the plane's."""
import functools

import numpy as np

from tests import mvs_cases as M

MAX_SOURCES = 8
REL_DEPTH_TOL, REPROJ_TOL, MAX_ANGLE_DEG, MAX_REL_JUMP = 0.01, 1.0, 30.0, 0.05


def normal_cos(angle_deg=MAX_ANGLE_DEG):
    """min_normal_cos as vggsfm_amd.fusion derives it"""
    import math
    return math.cos(math.radians(angle_deg))


def _nonzero(n):
    return (n[..., 0] != 0.0) | (n[..., 1] != 0.0) | (n[..., 2] != 0.0)


def world_point(pose, p0, p1, p2):
    """Q = P - t, X[i] = (R[0][i] Q[0] + R[1][i] Q[1]) + R[2][i] Q[2]"""
    q0, q1, q2 = p0 - pose[0, 3], p1 - pose[1, 3], p2 - pose[2, 3]
    return [(pose[0, i] * q0 + pose[1, i] * q1) + pose[2, i] * q2 for i in range(3)]


# ------------------------------------------------------------------------------------------------------- entry 2
def depth_normals(depth, poses, rays, ray_index, max_rel_jump=MAX_REL_JUMP):
    """-> dict: normals (S,H,W,3) float32 and the margins of every decision: jump (distance of |zn - z| from
    max_rel_jump z over the neighbours with depth), facing (|n . P|) and length (|n|) where a normal is formed."""
    S, H, W = depth.shape
    out = np.zeros((S, H, W, 3), np.float32)
    m_jump = m_facing = m_length = np.inf
    for s in range(S):
        z = depth[s].astype(np.float64)
        ray = rays[ray_index[s]]
        P = np.stack([ray[..., 0] * z, ray[..., 1] * z, z], -1)
        pad = np.zeros((H + 2, W + 2, 3))                                   # outside the frame: z = 0, never counts
        pad[1:-1, 1:-1] = P
        jump = max_rel_jump * z
        has = z > 0.0
        g = []
        for dx, dy in ((1, 0), (0, 1)):
            hi_p, lo_p = pad[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx], pad[1 - dy:H + 1 - dy, 1 - dx:W + 1 - dx]
            sides = []
            for nb in (hi_p, lo_p):
                zn = nb[..., 2]
                diff = np.abs(zn - z)
                sides.append((zn > 0.0) & (diff <= jump))
                both = (z > 0.0) & (zn > 0.0)
                m_jump = min(m_jump, float(np.abs(diff - jump)[both].min(initial=np.inf)))
            plus, minus = sides
            has = has & (plus | minus)
            g.append(np.where(plus[..., None], hi_p, P) - np.where(minus[..., None], lo_p, P))
        gx, gy = g
        n0 = gx[..., 1] * gy[..., 2] - gx[..., 2] * gy[..., 1]
        n1 = gx[..., 2] * gy[..., 0] - gx[..., 0] * gy[..., 2]
        n2 = gx[..., 0] * gy[..., 1] - gx[..., 1] * gy[..., 0]
        length = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
        d = (n0 * P[..., 0] + n1 * P[..., 1]) + n2 * P[..., 2]
        m_facing = min(m_facing, float(np.abs(d)[has].min(initial=np.inf)))
        m_length = min(m_length, float(length[has].min(initial=np.inf)))
        has = has & (length > 0.0) & ((d < 0.0) | (d > 0.0))
        with np.errstate(all="ignore"):
            m = [n0 / length, n1 / length, n2 / length]
        m = [np.where(d > 0.0, -c, c) for c in m]
        R = poses[s]
        for i in range(3):
            w = (R[0, i] * m[0] + R[1, i] * m[1]) + R[2, i] * m[2]
            out[s, ..., i] = np.where(has, w, 0.0).astype(np.float32)
    return {"normals": out, "margins": {"jump": m_jump, "facing": m_facing, "length": m_length}}


# ------------------------------------------------------------------------------------------------------- entry 3
def fuse_depth_maps(depth, poses, cams, rays, ray_index, sources, normals=None, colors=None, rel_depth_tol=REL_DEPTH_TOL,
                    reproj_tol=REPROJ_TOL, min_normal_cos=None, min_views=2, view_order=None):
    """The loop over the views with vggf_fuse_view restated per view -> dict: xyz (N,3) float64, normal, rgb (N,3) float32
    (zeros without normals / colours), num_views, view, pixel (N,) int32, claimed (S,H,W) uint8, counts (per fused view),
    seeds (per fused view), rejected_by_normal (sources that pass the geometric test and fail the normal test), and the
    margins: reproj, rel_depth, round (as mvs_cases.consistency_filter), front (|X[2]| of both transfers), normal
    (distance of the cosine from its limit where the test is made)."""
    S, H, W = depth.shape
    order = list(range(S)) if view_order is None else list(view_order)
    cos = normal_cos() if min_normal_cos is None else min_normal_cos
    claimed = np.zeros((S, H, W), np.uint8)
    ys0, xs0 = np.mgrid[0:H, 0:W].astype(np.float64)
    parts = {k: [] for k in ("xyz", "normal", "rgb", "num_views", "view", "pixel")}
    counts, seeds, rejected = [], [], 0
    mg = dict(reproj=np.inf, rel_depth=np.inf, round=np.inf, front=np.inf, normal=np.inf)
    for v in order:
        z = depth[v].astype(np.float64)
        seed = (z > 0.0) & (claimed[v] == 0)
        ray = rays[ray_index[v]]
        p0, p1 = ray[..., 0] * z, ray[..., 1] * z
        X = world_point(poses[v], p0, p1, z)
        nv = np.ones((H, W), np.int64)
        if normals is not None:
            n_seed = normals[v].astype(np.float64)
            seed_normal = _nonzero(n_seed)
            N = [np.where(seed_normal, n_seed[..., i], 0.0) for i in range(3)]
        if colors is not None:
            C = [colors[v, c].astype(np.float64) for c in range(3)]
        support = []
        for s in sources[v]:
            xs, ys, zc = M.transfer_project(M.relative_pose(poses[v], poses[s]), cams[s], p0, p1, z)
            with np.errstate(invalid="ignore"):
                xi, yi = np.floor(xs + 0.5), np.floor(ys + 0.5)
                front = seed & (zc > 0.0)
                go = front & M.inside_image(xi, yi, H, W)
            mg["front"] = min(mg["front"], float(np.abs(zc)[seed].min(initial=np.inf)))
            if front.any():
                fr = np.stack([xs[front] + 0.5, ys[front] + 0.5])
                mg["round"] = min(mg["round"], float(np.abs(fr - np.round(fr)).min()))
            xq, yq = np.where(go, xi, 0).astype(np.int64), np.where(go, yi, 0).astype(np.int64)
            zs = depth[s].astype(np.float64)[yq, xq]
            go = go & (zs > 0.0)
            rs = rays[ray_index[s]][yq, xq]
            q0, q1 = rs[..., 0] * zs, rs[..., 1] * zs
            xb, yb, zb = M.transfer_project(M.relative_pose(poses[s], poses[v]), cams[v], q0, q1, zs)
            mg["front"] = min(mg["front"], float(np.abs(zb)[go].min(initial=np.inf)))
            go = go & (zb > 0.0)
            with np.errstate(all="ignore"):
                ex, ey = xb - xs0, yb - ys0
                dist = np.sqrt(ex * ex + ey * ey)
                relz = np.abs(zb - z) / z
                near = go & (dist <= reproj_tol) & (relz <= rel_depth_tol)
            mg["reproj"] = min(mg["reproj"], float(np.abs(dist - reproj_tol)[go].min(initial=np.inf)))
            mg["rel_depth"] = min(mg["rel_depth"], float(np.abs(relz - rel_depth_tol)[go].min(initial=np.inf)))
            if normals is not None:
                ns = normals[s].astype(np.float64)[yq, xq]
                src_normal = _nonzero(ns)
                dot = (ns[..., 0] * n_seed[..., 0] + ns[..., 1] * n_seed[..., 1]) + ns[..., 2] * n_seed[..., 2]
                tested = near & seed_normal & src_normal
                mg["normal"] = min(mg["normal"], float(np.abs(dot - cos)[tested].min(initial=np.inf)))
                rejected += int((tested & ~(dot >= cos)).sum())
                near = near & (~tested | (dot >= cos))
                N = [np.where(near & src_normal, N[i] + ns[..., i], N[i]) for i in range(3)]
            Xs = world_point(poses[s], q0, q1, zs)
            X = [np.where(near, X[i] + Xs[i], X[i]) for i in range(3)]
            if colors is not None:
                C = [np.where(near, C[c] + colors[s, c].astype(np.float64)[yq, xq], C[c]) for c in range(3)]
            nv = nv + near
            support.append((s, near, yq, xq))
        emit = seed & (nv >= min_views)
        for s, near, yq, xq in support:
            hit = emit & near
            claimed[s][yq[hit], xq[hit]] = 1
        cnt = nv.astype(np.float64)
        idx = np.nonzero(emit.reshape(-1))[0]
        parts["xyz"].append(np.stack([(X[i] / cnt).reshape(-1)[idx] for i in range(3)], -1).reshape(-1, 3))
        if normals is not None:
            length = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
            with np.errstate(all="ignore"):
                unit = [np.where(length > 0.0, N[i] / length, 0.0).astype(np.float32) for i in range(3)]
            parts["normal"].append(np.stack([u.reshape(-1)[idx] for u in unit], -1).reshape(-1, 3))
        else:
            parts["normal"].append(np.zeros((len(idx), 3), np.float32))
        if colors is not None:
            parts["rgb"].append(np.stack([(C[c] / cnt).astype(np.float32).reshape(-1)[idx] for c in range(3)], -1).reshape(-1, 3))
        else:
            parts["rgb"].append(np.zeros((len(idx), 3), np.float32))
        parts["num_views"].append(nv.reshape(-1)[idx].astype(np.int32))
        parts["view"].append(np.full(len(idx), v, np.int32))
        parts["pixel"].append(idx.astype(np.int32))
        counts.append(len(idx))
        seeds.append(int(seed.sum()))
    empty = {"xyz": np.zeros((0, 3)), "normal": np.zeros((0, 3), np.float32), "rgb": np.zeros((0, 3), np.float32),
             "num_views": np.zeros(0, np.int32), "view": np.zeros(0, np.int32), "pixel": np.zeros(0, np.int32)}
    out = {k: np.concatenate([empty[k]] + parts[k]) for k in parts}
    out.update(claimed=claimed, counts=counts, seeds=seeds, rejected_by_normal=rejected, margins=mg)
    return out


# ------------------------------------------------------------------------------------------------------- the cases
def colours(frames):
    """(S,3,H,W) float32 planar colours from the scene's grey frames: three different rising functions of the grey value
    (their grey mix keeps 84 % of the texture's contrast, so the stereo sees what it sees on the grey frames)"""
    g = frames.astype(np.float32)
    return np.ascontiguousarray(np.stack([g, np.float32(0.8) * g + np.float32(0.1), np.float32(0.6) * g + np.float32(0.2)], 1))


def others(S):
    """every other view as a source, ascending"""
    return [[s for s in range(S) if s != v] for v in range(S)]


def _holes(depth, seed=3, share=0.15):
    out = depth.copy()
    out[np.random.default_rng(seed).random(out.shape) < share] = 0.0
    return out


@functools.lru_cache(maxsize=None)
def scenes():
    nine_x = (-0.8, -0.6, -0.4, -0.2, 0.0, 0.2, 0.4, 0.6, 0.8)
    return {"k0": M.scene(k=0.0), "k08": M.scene(k=0.08), "odd": M.scene(H=21, W=35, k=0.08), "nine": M.scene(xs=nine_x),
            "nine_k08": M.scene(xs=nine_x, k=0.08)}


def _depth(sc):
    return sc["truth"].astype(np.float32)


@functools.lru_cache(maxsize=None)
def normals_cases():
    """name -> arguments of depth_normals"""
    sc = scenes()
    mk = lambda s, d, **o: dict(dict(depth=d, poses=s["poses"], rays=s["rays"], ray_index=s["ray_index"],
                                     max_rel_jump=MAX_REL_JUMP), **o)
    step = _depth(sc["k08"]).copy()
    step[:, :, 16:] *= np.float32(1.2)                                      # half the map 20 % deeper: the jump test cuts
    b = sc["k08"]
    return {"k0_24x32": mk(sc["k0"], _depth(sc["k0"])), "k08_24x32": mk(b, _depth(b)),
            "k08_21x35": mk(sc["odd"], _depth(sc["odd"])), "holes": mk(b, _holes(_depth(b))), "depth_step": mk(b, step),
            "two_ray_maps": mk(b, _holes(_depth(b)), rays=np.concatenate([b["rays"], b["rays"]]),
                               ray_index=np.array([1, 0, 1], np.int32))}


@functools.lru_cache(maxsize=None)
def normals_reference(name):
    out = depth_normals(**normals_cases()[name])
    out["normals"].setflags(write=False)
    return out


def _scene_normals(sc, depth):
    return depth_normals(depth, sc["poses"], sc["rays"], sc["ray_index"], MAX_REL_JUMP)["normals"]


@functools.lru_cache(maxsize=None)
def fusion_cases():
    """name -> arguments of fuse_depth_maps (normals: the restated depth normals of the case's maps unless said)"""
    sc = scenes()

    def mk(s, depth=None, min_views=2, **over):
        d = _depth(s) if depth is None else depth
        S = d.shape[0]
        case = dict(depth=d, poses=s["poses"], cams=s["cams"], rays=s["rays"], ray_index=s["ray_index"], sources=others(S),
                    normals=_scene_normals(s, d), colors=colours(s["frames"]), rel_depth_tol=REL_DEPTH_TOL,
                    reproj_tol=REPROJ_TOL, min_normal_cos=normal_cos(), min_views=min_views, view_order=list(range(S)))
        case.update(over)
        return case

    b = sc["k08"]
    off = _holes(_depth(b))
    off[2] = np.where(off[2] > 0, off[2] * np.float32(1.06), 0).astype(np.float32)          # view 2 is 6 % off
    # the normals of view 1 turned by 40 degrees about the world's y axis: against the 30 degree limit the test decides
    a = np.radians(40.0)
    turn = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    tilted = _scene_normals(b, _depth(b)).copy()
    tilted[1] = (tilted[1].astype(np.float64) @ turn.T).astype(np.float32)
    away = dict(b, poses=b["poses"].copy())
    away["poses"][2] = np.diag([-1.0, 1.0, -1.0]) @ away["poses"][2]        # mvs_cases' facing_away: turned by 180 degrees
    copy = dict(b, poses=b["poses"].copy())
    copy["poses"][1] = copy["poses"][0]
    copy_depth = _depth(b).copy()
    copy_depth[1] = copy_depth[0]
    two = dict(b, rays=np.concatenate([b["rays"], b["rays"]]), ray_index=np.array([1, 0, 1], np.int32))
    return {
        "k0_mv1": mk(sc["k0"], min_views=1), "k0_mv2": mk(sc["k0"]), "k0_mv3": mk(sc["k0"], min_views=3),
        "k08_mv1": mk(b, min_views=1), "k08_mv2": mk(b), "k08_mv3": mk(b, min_views=3),
        "nine_views": mk(sc["nine"]), "nine_views_k08": mk(sc["nine_k08"], min_views=3),
        "k08_21x35": mk(sc["odd"]), "holes": mk(b, _holes(_depth(b))), "two_ray_maps": mk(two, _holes(_depth(b))),
        "off_mv1": mk(b, off, min_views=1), "off_mv2": mk(b, off),
        "tilted_normals": mk(b, normals=tilted), "no_normals": mk(b, normals=None), "no_colors": mk(b, colors=None),
        "zero_sources": mk(b, _holes(_depth(b)), min_views=1, sources=[[], [], []]),
        "facing_away": mk(away), "copy_of_view0": mk(copy, copy_depth),
        "order_201": mk(b, view_order=[2, 0, 1]), "order_012": mk(b, view_order=[0, 1, 2]),
        "all_zero": mk(b, np.zeros_like(_depth(b))),
    }


@functools.lru_cache(maxsize=None)
def fusion_reference(name):
    """the restatement of a case of fusion_cases() -- computed once, never modified"""
    out = fuse_depth_maps(**fusion_cases()[name])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------- against truth
def plane_distance(xyz):
    """distance of world points from the scene's plane"""
    p0, _, _, nrm = M._plane()
    return np.abs((xyz - p0) @ nrm)


def normal_angle_deg(normals):
    """angle between unit normals (..., 3) and the plane's normal, either sign; NaN for (0, 0, 0)"""
    _, _, _, nrm = M._plane()
    n = normals.astype(np.float64)
    s = np.linalg.norm(np.cross(n, nrm), axis=-1)                        # atan2: exact near 0, where arccos is not
    return np.where(_nonzero(n), np.degrees(np.arctan2(s, np.abs(n @ nrm))), np.nan)


TRUTH_CASES = ("k0_mv1", "k0_mv2", "k0_mv3", "k08_mv1", "k08_mv2", "k08_mv3", "nine_views", "nine_views_k08")

# measured on the restatement (tests/test_fusion_host.py prints them) over TRUTH_CASES, the true
# depth maps rounded to float32: the largest distance of a fused point from the plane and the largest angle between a depth
# normal and the plane's normal.  The CPU and the GPU tests assert 2 x these.
TRUTH_PLANE_DISTANCE, TRUTH_NORMAL_ANGLE_DEG = 2.3696e-7, 2.8715e-4
