"""Shared by the fundamental-matrix tests and oracle/gen_golden_fundamental.py: deterministic two-view scenes in hard
geometry (the regimes below), an independent 7-point solver and an independent 8-point fit in numpy long double (64-bit
mantissa), the admission rule that both decide alone, and the golden files' names, bounds and caps.

Neither reference shares a step with csrc/fundamental.hip or its mirror oracle/fundamental.py: the 7-point solver takes
its null space from an SVD of the 7x9 matrix (polished in long double), and finds the singular members of the pencil in a
rotated chart det(u G1 + G2) whose point at infinity is where |det| is largest, so that no solution can sit there; the
number of real solutions is the sign of the cubic's discriminant.  The 8-point fit takes the last right singular vector of
the N x 9 matrix itself (polished in long double) and enforces rank 2 from the singular vectors of the 3x3 matrix."""
import hashlib
import os

import numpy as np

from tests.essential_cases import distance, rodrigues, set_deviation  # noqa: F401  (re-exported to the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

CAP = 0.02                      # no solver-equality case leaves out more than this share of its samples or matches
JITTER, STABLE = 1e-13, 1e-7    # relative input perturbation; largest movement of an admitted sample's solution set
N_JITTER = 6
FLOOR7 = 1e-13                  # 7-point: deviation <= max(FLOOR7, sens)
FLOOR8, FACTOR8 = 1e-15, 100.0  # 8-point: deviation <= FACTOR8 * max(FLOOR8, eps / gap^2, sens)
BAND = 1e-3                     # relative band around the inlier threshold in which a match may fall on either side
CONSTRAINT = 1e-12              # reference self-check: |x2^T F x1| in its own normalised frame, |det|, at unit norm
N_MATCHES, N_SAMPLES = 200, 300
EIGHT_N = (8, 9, 63, 64, 65, 255, 256, 257, 513)
EIGHT_NOISE = (0.0, 0.3)
FLOW_N = (8, 65, 257, 600)
FLOW_H = 128
FLOW_LO = (0, 1, 2, 24, 3 * FLOW_H + 10)
SHALLOW_SPREAD = 3e-3           # depth spread of `shallow`: +-1e-3 leaves out 7 of 300 samples, +-3e-3 leaves out 4
NORM_EPS = 1e-8                 # the operation's own masked normalisation: sums / (n + 1e-8), sqrt(2) / (mean distance + 1e-8)

# name -> scene parameters.  `kind`: how the pose and the structure are drawn; `scale`: factor on the pixel coordinates
REGIMES = {
    "general": dict(kind="general"),
    "forward": dict(kind="forward"),
    "sideways": dict(kind="sideways", inverse_depth=(0.05, 0.4)),
    "vertical": dict(kind="vertical", inverse_depth=(0.05, 0.4)),
    "near_sideways_1e-11": dict(kind="sideways", disparity=1e-11, inverse_depth=(0.05, 0.4)),
    "near_sideways_1e-9": dict(kind="sideways", disparity=1e-9, inverse_depth=(0.05, 0.4)),
    "near_sideways_1e-7": dict(kind="sideways", disparity=1e-7, inverse_depth=(0.05, 0.4)),
    "lowpar": dict(kind="general", baseline=0.01),
    "offset": dict(kind="general", principal=1e5),
    "scaled_small": dict(kind="general", scale=1e-6),
    "scaled_large": dict(kind="general", scale=1e3),
    "shallow": dict(kind="general", depth=SHALLOW_SPREAD),
    "planar80": dict(kind="general", planar=0.8),
    "planar": dict(kind="general", planar=1.0),
    "rotation": dict(kind="rotation"),
    "identical": dict(kind="identical"),
}
EQUALITY = tuple(n for n in REGIMES if n not in ("planar80", "planar", "rotation", "identical"))
DEGENERATE = ("planar80", "planar", "rotation", "identical")
FLOW_BATCHES = {                # one threshold per batch, so the scaled regimes travel with themselves
    "mixed": (("general", 0), ("forward", 0), ("sideways", 0)),
    "hard": (("near_sideways_1e-9", 0), ("lowpar", 0), ("offset", 0)),
    "planar": (("planar80", 0), ("general", 1), ("near_sideways_1e-11", 0)),
    "small": (("scaled_small", 0), ("scaled_small", 1)),
    "large": (("scaled_large", 0), ("scaled_large", 1)),
}
# pixels at scale 1.  The inliers are exact, so the threshold can be tight; it has to be, and the clearance wide, for the
# true inlier set to be the only right answer: at 1 px and 5 px a matrix that keeps every exact inlier within 0.1 px and
# takes in one or two outliers as well exists in `forward`, `lowpar` (whose whole parallax is 1.5 px) and `scaled_small`,
# and LO-RANSAC rightly prefers it
FLOW_MAX_ERROR, FLOW_CLEARANCE = 0.01, 50.0


def path(name):
    return os.path.join(GOLDEN, f"fundamental_{name}.npz")


def load(name):
    with np.load(path(name)) as z:
        return {k: z[k] for k in z.files}


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _seed(name, salt):
    return [int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little"), salt]


# --- long-double geometry ----------------------------------------------------------------------------------------------
def _homog(p):
    p = np.asarray(p, LD)
    return np.concatenate([p, np.ones((len(p), 1), LD)], 1)


def sampson_sq(F, p1, p2):
    """Long-double squared Sampson distance of (N,2) points under (...,3,3) matrices (x2^T F x1 = 0) -> (...,N)."""
    F, h1, h2 = np.asarray(F, LD), _homog(p1), _homog(p2)
    l = np.einsum("...ij,nj->...ni", F, h1)
    m = np.einsum("...ji,nj->...ni", F, h2)
    num = np.einsum("...ni,ni->...n", l, h2) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        r = num / (l[..., 0] ** 2 + l[..., 1] ** 2 + m[..., 0] ** 2 + m[..., 1] ** 2)
    return np.where(np.isfinite(r), r, LD(1e6))


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], LD)


def true_fundamental(R, t, K1, K2):
    F = np.linalg.inv(K2.astype(np.float64)).T.astype(LD) @ _skew(t) @ np.asarray(R, LD) @ np.linalg.inv(K1.astype(np.float64)).astype(LD)
    n = np.sqrt((F * F).sum())
    return (F / n).astype(np.float64) if n > 0 else np.zeros((3, 3))


# --- scenes ----------------------------------------------------------------------------------------------------------------
def scene(name, N=N_MATCHES, outliers=0.0, noise=0.0, salt=0, clearance=FLOW_CLEARANCE, spread_outliers=False):
    """One pair of the regime `name`: dict(x1, x2 (N,2) pixels, F (3,3) true matrix of unit norm [zeros where there is
    none], inl (N,) bool, scale).  Outliers are drawn again until their Sampson distance to the true F exceeds `clearance`
    pixels (at scale 1); with spread_outliers they are every match n with n % 10 in (1, 4, 7), else the first ones."""
    p = REGIMES[name]
    rng = np.random.default_rng(_seed(name, salt))
    kind, f = p["kind"], 1000.0
    pp = p.get("principal", 500.0)
    K = np.array([[f, 0, pp], [0, f, pp], [0, 0, 1.0]])
    R, t = rodrigues(rng.uniform(-0.25, 0.25, 3) + 1e-3), rng.normal(size=3)
    t /= np.linalg.norm(t)
    if kind == "forward":
        R, t = rodrigues(rng.uniform(-0.02, 0.02, 3) + 1e-3), np.array([0.0, 0.0, 1.0])
    elif kind in ("sideways", "vertical"):
        R, t = np.eye(3), np.array([1.0, 0.0, 0.0]) if kind == "sideways" else np.array([0.0, 1.0, 0.0])
    elif kind == "rotation":
        t = np.zeros(3)
    elif kind == "identical":
        R, t = np.eye(3), np.zeros(3)
    t = t * p.get("baseline", 1.0)
    depth = p.get("depth", 2.5)
    X = np.stack([rng.uniform(-2, 2, N), rng.uniform(-2, 2, N), 6.5 + rng.uniform(-depth, depth, N)], 1)
    if "inverse_depth" in p:                   # image positions and inverse depths drawn evenly: disparities vary widely
        lo, hi = p["inverse_depth"]
        Z = 1.0 / rng.uniform(lo, hi, N)
        X = np.stack([rng.uniform(-0.4, 0.4, N) * Z, rng.uniform(-0.4, 0.4, N) * Z, Z], 1)
    if "planar" in p:
        on = rng.random(N) < p["planar"] if p["planar"] < 1 else np.ones(N, bool)
        nrm = np.array([0.2, -0.1, 1.0])
        X[on, 2] = (6.5 - X[on, :2] @ nrm[:2]) / nrm[2]
    Y = X @ R.T + t
    x1 = X[:, :2] / X[:, 2:] * f + pp
    x2 = Y[:, :2] / Y[:, 2:] * f + pp
    if kind == "sideways":
        x2[:, 1] = x1[:, 1] + p.get("disparity", 0.0) * rng.normal(size=N)
    elif kind == "vertical":
        x2[:, 0] = x1[:, 0]
    elif kind == "identical":
        x2 = x1.copy()
    F = true_fundamental(R, t, K, K)
    if noise > 0:
        x1 = x1 + noise * rng.normal(size=(N, 2))
        x2 = x2 + noise * rng.normal(size=(N, 2))
    inl = np.ones(N, bool)
    if outliers > 0:
        if spread_outliers:
            inl = ~np.isin(np.arange(N) % 10, (1, 4, 7))
        else:
            inl[:int(round(outliers * N))] = False
        for n in np.nonzero(~inl)[0]:
            for attempt in range(10000):        # (a match next to the epipole is near every epipolar line: move it too)
                if attempt % 20 == 19:
                    x1[n] = pp + f * rng.uniform(-0.5, 0.5, 2)
                x2[n] = pp + f * rng.uniform(-0.5, 0.5, 2)
                if not F.any() or float(sampson_sq(F, x1[n:n + 1], x2[n:n + 1])[0]) > clearance ** 2:
                    break
    s = p.get("scale", 1.0)
    if s != 1.0:
        x1, x2 = x1 * s, x2 * s
        Ks = np.diag([s, s, 1.0]) @ K
        F = true_fundamental(R, t, Ks, Ks)
    return dict(x1=np.ascontiguousarray(x1), x2=np.ascontiguousarray(x2), F=F, inl=inl, scale=s)


def draw_samples(name, N=N_MATCHES, H=N_SAMPLES, among=None):
    """(H,7) int32 samples without repetition, from the indices `among` (default: all N)."""
    rng = np.random.default_rng(_seed(name, 7))
    pool = np.arange(N) if among is None else np.asarray(among)
    return np.stack([rng.choice(pool, 7, replace=False) for _ in range(H)]).astype(np.int32)


# --- the independent references --------------------------------------------------------------------------------------------
def _hartley(p, eps=0.0):
    """p (n,2) long double -> normalised points, T (3,3): centroid to the origin, mean distance sqrt(2).  With eps the
    frame is the one the 8-point operation is defined in (NORM_EPS): a least-squares fit on noisy matches depends on its
    frame, an exact null space does not."""
    n = LD(len(p)) + LD(eps)
    c = p.sum(0) / n
    d = np.sqrt(((p - c) ** 2).sum(1)).sum() / n
    s = np.sqrt(LD(2)) / (d + LD(eps))
    T = np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]], LD)
    return (p - c) * s, T


def _design(q1, q2):
    one = np.ones(len(q1), LD)
    return np.stack([q2[:, 0] * q1[:, 0], q2[:, 0] * q1[:, 1], q2[:, 0], q2[:, 1] * q1[:, 0], q2[:, 1] * q1[:, 1], q2[:, 1],
                     q1[:, 0], q1[:, 1], one], 1)


def _det_coefficients(G1, G2):
    """Coefficients q[k] of u^k in det(u G1 + G2): the determinant is linear in each row, k rows come from G1."""
    q = np.zeros(4, LD)
    for pick in range(8):
        rows = [G1[i] if pick >> i & 1 else G2[i] for i in range(3)]
        q[bin(pick).count("1")] += rows[0] @ np.cross(rows[1], rows[2])
    return q


def _finish(Fh, T1, T2):
    F = T2.T @ Fh @ T1
    return F / np.sqrt((F * F).sum())


def seven_point_ref(p1, p2, with_frames=False):
    """p1, p2 (7,2) -> (k,3,3) float64 unit-norm solutions, k in 0..3 (x2^T F x1 = 0).  with_frames: also the long-double
    solutions in the normalised frame and the 7x9 matrix (for the self-checks)."""
    with np.errstate(all="ignore"):
        q1, T1 = _hartley(np.asarray(p1, LD))
        q2, T2 = _hartley(np.asarray(p2, LD))
        A = _design(q1, q2)
        empty = (np.zeros((0, 3, 3)), np.zeros((0, 3, 3), LD), A) if with_frames else np.zeros((0, 3, 3))
        if not np.isfinite(A).all():
            return empty
        A64 = A.astype(np.float64)
        Nb = np.linalg.svd(A64)[2][7:].T.astype(LD)                      # (9,2)
        Ap = np.linalg.pinv(A64).astype(LD)
        for _ in range(3):                                               # residual in long double, correction in double
            Nb = Nb - Ap @ (A @ Nb)
        Nb[:, 0] /= np.sqrt(Nb[:, 0] @ Nb[:, 0])
        Nb[:, 1] -= (Nb[:, 1] @ Nb[:, 0]) * Nb[:, 0]
        Nb[:, 1] /= np.sqrt(Nb[:, 1] @ Nb[:, 1])
        F1, F2 = Nb[:, 0].reshape(3, 3), Nb[:, 1].reshape(3, 3)
        # rotate the pencil so that its point at infinity is where |det| is largest: no solution sits there
        ang = np.arange(8) * (np.pi / 8)
        dets = [abs(np.linalg.det((np.cos(a) * F1 + np.sin(a) * F2).astype(np.float64))) for a in ang]
        a = LD(ang[int(np.argmax(dets))])
        G1, G2 = np.cos(a) * F1 + np.sin(a) * F2, -np.sin(a) * F1 + np.cos(a) * F2
        q = _det_coefficients(G1, G2)
        if not (np.isfinite(q).all() and q[3] != 0):
            return empty
        d, c, b, a3 = q
        disc = 18 * a3 * b * c * d - 4 * b ** 3 * d + b * b * c * c - 4 * a3 * c ** 3 - 27 * a3 * a3 * d * d
        r = np.roots(q[::-1].astype(np.float64))
        if len(r) != 3:
            return empty
        us = r.real if disc > 0 else r.real[[int(np.argmin(np.abs(r.imag)))]]
        sols, frames = [], []
        for u in us.astype(LD):
            for _ in range(4):                                           # Newton polish in long double
                f, df = ((a3 * u + b) * u + c) * u + d, (3 * a3 * u + 2 * b) * u + c
                if df != 0 and np.isfinite(f / df):
                    u = u - f / df
            Fh = u * G1 + G2
            Fh = Fh / np.sqrt((Fh * Fh).sum())
            frames.append(Fh)
            sols.append(_finish(Fh, T1, T2).astype(np.float64))
        S = np.array(sols).reshape(-1, 3, 3)
        if not np.isfinite(S).all():
            return empty
    return (S, np.array(frames, LD).reshape(-1, 3, 3), A) if with_frames else S


def _polish_smallest(A, V, s):
    """The right singular vector of A's smallest singular value: from the double SVD (V columns, s), polished against the
    long-double residual of A^T A in the double eigenbasis."""
    n = V.shape[1]
    v = V[:, n - 1].astype(LD)
    Vl = V.astype(LD)
    s2 = np.zeros(n, LD)
    s2[:len(s)] = s.astype(LD) ** 2
    for _ in range(4):
        g = A.T @ (A @ v)
        rho = v @ g
        res = g - rho * v
        den = s2[:n - 1] - rho
        if not (den != 0).all():
            break
        v = v - Vl[:, :n - 1] @ ((Vl[:, :n - 1].T @ res) / den)
        v = v / np.sqrt(v @ v)
    return v


def eight_point_ref(x1, x2, mask=None):
    """x1, x2 (N,2); mask (N,) bool -> (F (3,3) float64 unit norm or None, gap = sigma_8 / sigma_1 of the normalised
    design matrix)."""
    with np.errstate(all="ignore"):
        sel = np.ones(len(x1), bool) if mask is None else np.asarray(mask, bool)
        if sel.sum() < 8:
            return None, 0.0
        q1, T1 = _hartley(np.asarray(x1, LD)[sel], NORM_EPS)
        q2, T2 = _hartley(np.asarray(x2, LD)[sel], NORM_EPS)
        A = _design(q1, q2)
        if not np.isfinite(A).all():
            return None, 0.0
        _, s, Vt = np.linalg.svd(A.astype(np.float64), full_matrices=True)
        gap = float(s[7] / s[0])
        Fh = _polish_smallest(A, Vt.T, s).reshape(3, 3)
        _, s3, V3t = np.linalg.svd(Fh.astype(np.float64))
        v3 = _polish_smallest(Fh, V3t.T, s3)
        Fh = Fh - np.outer(Fh @ v3, v3)                                  # = U diag(s1, s2, 0) V^T
        F = _finish(Fh, T1, T2).astype(np.float64)
    return (F if np.isfinite(F).all() else None), gap


def _jitters(shape, key):
    rng = np.random.default_rng([key, 99])
    return [1.0 + JITTER * rng.normal(size=shape) for _ in range(N_JITTER)]


def admit_seven(p1, p2, key):
    """-> (solutions (k,3,3), admitted, sens): the reference alone decides.  Admitted: the same number of real
    solutions under every relative perturbation of JITTER, and the set moves by at most STABLE (its movement is sens)."""
    S = seven_point_ref(p1, p2)
    sens, same = 0.0, True
    for j1, j2 in zip(_jitters(p1.shape, key), _jitters(p2.shape, key + 1)):
        Sj = seven_point_ref(p1 * j1, p2 * j2)
        same = same and len(Sj) == len(S)
        sens = max(sens, set_deviation(S, Sj))
    return S, bool(same and sens <= STABLE and len(S) > 0), float(sens)


def admit_eight(x1, x2, mask, key):
    """-> (F or None, gap, admitted, sens) of the 8-point fit, by the same rule."""
    F, gap = eight_point_ref(x1, x2, mask)
    if F is None:
        return None, gap, False, np.inf
    sens = 0.0
    for j1, j2 in zip(_jitters(x1.shape, key), _jitters(x2.shape, key + 1)):
        Fj, _ = eight_point_ref(x1 * j1, x2 * j2, mask)
        sens = max(sens, np.inf if Fj is None else float(distance(F, Fj)))
    return F, gap, bool(sens <= STABLE), float(sens)


def bound8(gap, sens):
    return FACTOR8 * max(FLOOR8, EPS / gap ** 2 if gap > 0 else np.inf, sens)


# --- golden cases ----------------------------------------------------------------------------------------------------------
def eight_masks(name, N):
    """(2,N) bool: every match, and about 70 % (never fewer than 8)."""
    rng = np.random.default_rng(_seed(name, 1000 + N))
    m = rng.random(N) < 0.7
    need = 8 - int(m.sum())
    if need > 0:
        m[np.nonzero(~m)[0][:need]] = True
    return np.stack([np.ones(N, bool), m])


def build_regime(name, samples=None):
    """Everything fundamental_<name>.npz holds.  `samples` (rows of the stored sample list) restricts the 7-point part, for
    the regeneration check."""
    sc = scene(name)
    smp = draw_samples(name)
    rows = range(N_SAMPLES) if samples is None else samples
    sol = np.zeros((len(rows), 3, 3, 3))
    cnt, sens, adm = np.zeros(len(rows), np.int64), np.zeros(len(rows)), np.zeros(len(rows), bool)
    for i, h in enumerate(rows):
        S, adm[i], sens[i] = admit_seven(sc["x1"][smp[h]], sc["x2"][smp[h]], 2 * h)
        cnt[i] = len(S)
        sol[i, :len(S)] = S
    out = dict(x1=sc["x1"], x2=sc["x2"], F_true=sc["F"], samples=smp, ref_F=sol, ref_count=cnt, sens=sens, admit=adm)
    if samples is not None or name not in EQUALITY:
        return out
    nmax = max(EIGHT_N)
    e_F, e_gap, e_sens, e_adm = (np.zeros((len(EIGHT_NOISE), len(EIGHT_N), 2) + s) for s in ((3, 3), (), (), ()))
    for a, noise in enumerate(EIGHT_NOISE):
        big = scene(name, N=nmax, noise=noise, salt=50)
        out[f"e_x1_{a}"], out[f"e_x2_{a}"] = big["x1"], big["x2"]
        for b, N in enumerate(EIGHT_N):
            for c, m in enumerate(eight_masks(name, N)):
                F, e_gap[a, b, c], e_adm[a, b, c], e_sens[a, b, c] = admit_eight(big["x1"][:N], big["x2"][:N], m, 7 * N + c)
                e_F[a, b, c] = 0.0 if F is None else F
    out.update(e_F=e_F, e_gap=e_gap, e_sens=e_sens, e_admit=e_adm.astype(bool))
    return out


def flow_scene(name, salt, N):
    """Inliers exact, 30 % outliers with clearance spread over the matches (none at N = 8, where eight inliers are the
    least an 8-point fit is defined on), thresholds scaled with the coordinates."""
    sc = scene(name, N=N, outliers=0.3 if N > 8 else 0.0, salt=100 + salt, spread_outliers=True)
    sc["max_error"] = FLOW_MAX_ERROR * sc["scale"]
    return sc


def flow_samples(batch, N, inl_all):
    """(FLOW_H,7): the first 8 samples lie in every pair's true inliers, the rest anywhere."""
    common = np.nonzero(np.all(inl_all, 0))[0]
    head = draw_samples(f"flow_{batch}_{N}", N, 8, among=common)
    return np.concatenate([head, draw_samples(f"flow_{batch}_{N}_rest", N, FLOW_H - 8)])


def flow_masks(batch, N, B):
    """[None, all true, about 90 %] valid masks (B,N)."""
    rng = np.random.default_rng(_seed(f"mask_{batch}", N))
    return [None, np.ones((B, N), bool), rng.random((B, N)) < 0.9]


def build_flow():
    """fundamental_flow.npz: per pair of every flow batch and N, the reference's 8-point fit on the true inliers (all of
    them, and those the 90 % mask keeps), its gap and sens, the share of matches inside the band, and the input digest."""
    out = {}
    for batch, pairs in FLOW_BATCHES.items():
        for N in FLOW_N:
            scs = [flow_scene(n, s, N) for n, s in pairs]
            masks = flow_masks(batch, N, len(pairs))
            for b, sc in enumerate(scs):
                for tag, vm in (("all", np.ones(N, bool)), ("m90", masks[2][b])):
                    use = sc["inl"] & vm
                    F, gap, adm, sens = admit_eight(sc["x1"], sc["x2"], use, N + b)
                    key = f"{batch}_{N}_{b}_{tag}"
                    thr = LD(sc["max_error"]) ** 2
                    if F is None:
                        out[key + "_F"], band = np.zeros((3, 3)), 0.0
                    else:
                        r = sampson_sq(F, sc["x1"], sc["x2"])
                        band = float((np.abs(r - thr) <= BAND * thr).mean())
                        out[key + "_F"] = F
                    out[key + "_meta"] = np.array([gap, sens, band, float(adm), float(use.sum())])
                out[f"{batch}_{N}_{b}_digest"] = np.array(digest(sc["x1"], sc["x2"], sc["inl"]))
    return out


# --- the checks the CPU tests (on the mirror) and the GPU tests (on the kernels) share ----------------------------------------
def unit(F):
    return F / np.linalg.norm(F, axis=(-2, -1), keepdims=True)


def check_seven(g, F, valid):
    """F (H,3,3,3), valid (H,3) of a solver on the golden samples of one regime -> (largest deviation / max(FLOOR7, sens),
    list of failures): on every admitted sample the reference's number of real solutions and its solutions."""
    worst, bad = 0.0, []
    for h in np.nonzero(g["admit"])[0]:
        S, M = g["ref_F"][h, :g["ref_count"][h]], F[h][valid[h].astype(bool)]
        if len(S) != len(M):
            missing = S[distance(S[:, None], M[None]).min(1) > 1e-6] if len(M) else S
            bad.append(f"sample {h}: {len(M)} solutions, the reference has {len(S)}; missing\n{missing}")
            continue
        dev, lim = set_deviation(S, M), max(FLOOR7, g["sens"][h])
        worst = max(worst, dev / lim)
        if not dev <= lim:
            bad.append(f"sample {h}: deviation {dev:.3e} > {lim:.3e}")
    return worst, bad


def eight_cases(g, name):
    """Yield (label, x1, x2, mask (N,), F_ref, gap, sens) of every admitted 8-point case of the regime's golden file."""
    for a, noise in enumerate(EIGHT_NOISE):
        for b, N in enumerate(EIGHT_N):
            for c, m in enumerate(eight_masks(name, N)):
                if g["e_admit"][a, b, c]:
                    yield (f"noise {noise} N {N} mask {'full' if c == 0 else '70%'}", g[f"e_x1_{a}"][:N], g[f"e_x2_{a}"][:N], m,
                           g["e_F"][a, b, c], float(g["e_gap"][a, b, c]), float(g["e_sens"][a, b, c]))


def check_flow(g, batch, N, b, sc, vm, lo, F, num, mask):
    """One pair's result of the whole flow against the golden reference fit.  Returns the figures it asserted on."""
    full = vm is None or bool(np.all(vm))
    key = f"{batch}_{N}_{b}_{'all' if full else 'm90'}"
    Fref, (gap, sens, band, adm, nuse) = g[key + "_F"], g[key + "_meta"]
    usable = sc["inl"] & (np.ones(N, bool) if vm is None else vm)
    assert int(nuse) == int(usable.sum())
    assert int(num) == int(mask.sum()), (key, lo)
    assert F[2, 2] == 1.0 or (abs(F[2, 2]) <= 1e-8 and abs(np.linalg.norm(F) - 1) < 1e-12), (key, lo, F)
    out = dict(key=key, lo=lo, band=band, dev=None, bound=None)
    if not adm:                                 # fewer than 8 usable inliers, or a fit the reference itself cannot pin
        return out
    assert band <= CAP, (key, band)
    thr = LD(sc["max_error"]) ** 2
    outside = np.abs(sampson_sq(Fref, sc["x1"], sc["x2"]) - thr) > BAND * thr
    wrong = np.nonzero((mask != usable) & outside)[0]
    assert len(wrong) == 0, (key, lo, wrong)
    if lo >= 1:
        out["dev"], out["bound"] = float(distance(unit(F), Fref)), bound8(gap, sens)
        assert out["dev"] <= out["bound"], (key, lo, out)
    return out
