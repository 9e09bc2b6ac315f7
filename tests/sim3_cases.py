"""The yardstick of the Sim(3) kernels (csrc/sim3.hip) and its cases: weighted Umeyama, hypothesis scoring, the ranking
rule, the LO loop and the all-pairs pose errors restated in ``np.longdouble`` (numpy's linalg has no long double, so the
3x3 decompositions are hand-written Jacobi iterations), a float64 ``np.linalg.svd`` Umeyama as the second opinion and as
the measure of what float64 can give, and every case with its seed.  tests/test_sim3_reference.py checks all of this by
itself on the CPU; tests/test_gpu_sim3.py compares the device with it.

Convention: tgt ~ s R src + t.  A transform is (s, R (3,3), t (3,))."""
import numpy as np

LD = np.longdouble
COLLINEAR = 1e-12          # second / first eigenvalue of the source scatter at or below which a set is collinear
NEAR = 1e-9                # a residual within NEAR * max_error^2 of the threshold could be classified either way
EPS = 1e-15                # the reference's clamp in rotation_angle and compare_translation_by_angle


# --- 3x3 decompositions in any dtype -----------------------------------------------------------------------------------
def _rotation(app, aqq, apq, dt):
    if apq == 0:
        return dt(1), dt(0)
    with np.errstate(over="ignore"):                       # (a huge tau is a rotation by nothing)
        tau = (aqq - app) / (2 * apq)
        t = (dt(1) if tau >= 0 else dt(-1)) / (abs(tau) + np.hypot(dt(1), tau))
    c = 1 / np.sqrt(1 + t * t)
    return c, t * c


def sym_eigenvalues(A, sweeps=30):
    """Eigenvalues of a symmetric 3x3 matrix, descending (two-sided cyclic Jacobi in A's dtype)."""
    A = np.array(A)
    dt = A.dtype.type
    for _ in range(sweeps):
        for p in range(2):
            for q in range(p + 1, 3):
                c, s = _rotation(A[p, p], A[q, q], A[p, q], dt)
                J = np.eye(3, dtype=A.dtype)
                J[p, p], J[q, q], J[p, q], J[q, p] = c, c, s, -s
                A = J.T @ A @ J
    return np.sort(np.diag(A))[::-1]


def svd3(C, sweeps=30):
    """C = U diag(S) V^T by one-sided Jacobi in C's dtype: returns (A = C V with columns in descending norm, S, V)."""
    A, V = np.array(C), np.eye(3, dtype=C.dtype)
    dt = A.dtype.type
    for _ in range(sweeps):
        for p in range(2):
            for q in range(p + 1, 3):
                c, s = _rotation(A[:, p] @ A[:, p], A[:, q] @ A[:, q], A[:, p] @ A[:, q], dt)
                for M in (A, V):
                    mp, mq = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = c * mp - s * mq, s * mp + c * mq
    norms = np.sqrt((A * A).sum(0))
    order = np.argsort(-norms, kind="stable")
    return A[:, order], norms[order], V[:, order]


def identity(dt=LD):
    return dt(1), np.eye(3, dtype=dt), np.zeros(3, dtype=dt)


def umeyama(src, tgt, weights=None, estimate_scale=True, dt=LD):
    """(s, R, t, valid) of one problem in dtype `dt`; the rules of vggs_sim3_fit."""
    src, tgt = np.asarray(src, dt), np.asarray(tgt, dt)
    w = np.ones(len(src), dt) if weights is None else np.asarray(weights, dt)
    w = np.where(w > 0, w, 0)
    keep = w > 0
    if keep.sum() < 3:
        return identity(dt) + (False,)
    src, tgt, w = src[keep], tgt[keep], w[keep]
    W = w.sum()
    mu_s, mu_t = (w[:, None] * src).sum(0) / W, (w[:, None] * tgt).sum(0) / W
    ds, dtg = src - mu_s, tgt - mu_t
    Sigma = (w[:, None, None] * dtg[:, :, None] * ds[:, None, :]).sum(0) / W
    scatter = (w[:, None, None] * ds[:, :, None] * ds[:, None, :]).sum(0) / W
    var = np.trace(scatter)
    if not var > 0:
        return identity(dt) + (False,)
    ev = sym_eigenvalues(scatter)
    if not ev[1] > dt(COLLINEAR) * ev[0]:
        return identity(dt) + (False,)
    A, S, V = svd3(Sigma)
    if not (S[0] > 0 and S[1] > 0):
        return identity(dt) + (False,)
    u1, u2 = A[:, 0] / S[0], A[:, 1] / S[1]
    u3 = np.cross(u1, u2)
    sd = dt(1) if np.linalg.det(V.astype(np.float64)) >= 0 else dt(-1)
    R = np.outer(u1, V[:, 0]) + np.outer(u2, V[:, 1]) + sd * np.outer(u3, V[:, 2])
    trace = S[0] + S[1] + sd * (A[:, 2] @ u3)
    s = trace / var if estimate_scale else dt(1)
    t = mu_t - s * (R @ mu_s)
    if not (np.isfinite(s) and s > 0 and np.isfinite(R).all() and np.isfinite(t).all()):
        return identity(dt) + (False,)
    return s, R, t, True


def umeyama_f64(src, tgt, weights=None, estimate_scale=True):
    """The textbook float64 evaluation with np.linalg.svd (Umeyama 1991), no validity rules: what float64 gives."""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    w = np.ones(len(src)) if weights is None else np.asarray(weights, np.float64)
    W = w.sum()
    mu_s, mu_t = (w[:, None] * src).sum(0) / W, (w[:, None] * tgt).sum(0) / W
    ds, dtg = src - mu_s, tgt - mu_t
    Sigma = (w[:, None] * dtg).T @ ds / W
    var = (w * (ds * ds).sum(1)).sum() / W
    U, S, Vt = np.linalg.svd(Sigma)
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0])
    R = U @ D @ Vt
    s = (S * np.diag(D)).sum() / var if estimate_scale else 1.0
    return s, R, mu_t - s * R @ mu_s


def fit_deviation(got, ref, src, weights=None):
    """(relative |ds|, max |dR|, |dt| relative to |t| + s * extent) of transform `got` against `ref`."""
    s, R, t = (np.asarray(x, LD) for x in got)
    s0, R0, t0 = ref
    w = np.ones(len(src)) if weights is None else np.asarray(weights, np.float64)
    pts = np.asarray(src, LD)[w > 0]
    extent = np.sqrt(((pts - pts.mean(0)) ** 2).sum(1)).max()
    return (float(abs(s - s0) / s0), float(np.abs(R - R0).max()),
            float(np.sqrt(((t - t0) ** 2).sum()) / (np.sqrt((t0 ** 2).sum()) + s0 * extent)))


# --- scoring, ranking, LO ---------------------------------------------------------------------------------------------
def residuals(T, src, tgt, dt=LD):
    s, R, t = T
    d = np.asarray(tgt, dt) - (dt(s) * (np.asarray(src, dt) @ np.asarray(R, dt).T) + np.asarray(t, dt))
    return (d * d).sum(1)


def score(T, src, tgt, mask, max_error, dt=LD):
    """(count, sum of the inliers' squared residuals, inlier mask, residuals)."""
    r = residuals(T, src, tgt, dt)
    inl = r <= dt(max_error) ** 2
    if mask is not None:
        inl &= np.asarray(mask, bool)
    return int(inl.sum()), r[inl].sum(), inl, r


def near_threshold(r, mask, max_error):
    """Points whose residual is within NEAR * max_error^2 of the threshold."""
    thr = LD(max_error) ** 2
    near = np.abs(r - thr) <= LD(NEAR) * thr
    return near if mask is None else near & np.asarray(mask, bool)


def ranks_before(c1, s1, i1, c2, s2, i2):
    """The project's rule: more inliers, then the smaller inlier residual sum, then the lower index."""
    if c1 != c2:
        return c1 > c2
    if s1 != s2:
        return s1 < s2
    return i1 < i2


def rank_best(counts, sums):
    """Index of the winner among hypotheses with count >= 0, or -1."""
    best = -1
    for h in range(len(counts)):
        if counts[h] >= 0 and (best < 0 or ranks_before(counts[h], sums[h], h, counts[best], sums[best], best)):
            best = h
    return best


def sample_transform(src, tgt, mask, idx, estimate_scale=True, dt=LD):
    """The minimal hypothesis of three point indices, (s, R, t, valid)."""
    i = [int(k) for k in idx]
    n = len(src)
    if len(set(i)) < 3 or min(i) < 0 or max(i) >= n or (mask is not None and not np.asarray(mask, bool)[i].all()):
        return identity(dt) + (False,)
    return umeyama(np.asarray(src)[i], np.asarray(tgt)[i], None, estimate_scale, dt)


def local_optimisation(T, src, tgt, mask, max_error, rounds, estimate_scale=True):
    """The LO loop of vggs_sim3_ransac from transform T.  Returns (T, count, sum, mask, accepted, history) where history
    holds one (mask, residuals) per scored transform, the incoming one first."""
    count, rsum, inl, r = score(T, src, tgt, mask, max_error)
    history, accepted = [(inl, r)], 0
    for _ in range(rounds):
        s, R, t, ok = umeyama(src, tgt, inl.astype(np.float64), estimate_scale)
        if not ok:
            break
        c2, s2, inl2, r2 = score((s, R, t), src, tgt, mask, max_error)
        history.append((inl2, r2))
        if not (c2 > count or (c2 == count and s2 < rsum)):
            break
        same = np.array_equal(inl2, inl)
        T, count, rsum, inl, accepted = (s, R, t), c2, s2, inl2, accepted + 1
        if same:
            break
    return T, count, rsum, inl, accepted, history


# --- pair errors ----------------------------------------------------------------------------------------------------------
def pair_errors(pred, gt, dt=LD):
    """(rotation error, translation-direction error) in degrees of all pairs i < j (torch.combinations order) of (S,3,4)
    world-to-camera poses, by the definitions of the reference's rotation_angle / translation_angle."""
    pred, gt = np.asarray(pred, dt), np.asarray(gt, dt)
    S = len(gt)
    deg = dt(180) / (LD("3.14159265358979323846264338327950288") if dt is LD else dt(np.pi))
    rot, trans = [], []
    for i in range(S):
        for j in range(i + 1, S):
            rel = []
            for P in (gt, pred):
                R = P[j, :, :3] @ P[i, :, :3].T
                rel.append((R, P[j, :, 3] - R @ P[i, :, 3]))
            d2 = (1 + (rel[0][0] * rel[1][0]).sum()) / 4
            rot.append(np.arccos(1 - 2 * max(1 - d2, dt(EPS))) * deg)
            tg = rel[0][1] / (np.sqrt((rel[0][1] ** 2).sum()) + dt(EPS))
            tp = rel[1][1] / (np.sqrt((rel[1][1] ** 2).sum()) + dt(EPS))
            a = np.arccos(np.sqrt(1 - max(1 - (tg @ tp) ** 2, dt(EPS))))
            a = (a if np.isfinite(a) else dt(1e6)) * deg
            trans.append(min(a, abs(180 - a)))
    return np.array(rot, dt), np.array(trans, dt)


# --- cases ------------------------------------------------------------------------------------------------------------
def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def _moved(rng, src, scale, offset=0.0, noise=0.0):
    R, t = random_rotation(rng), rng.normal(size=3) + offset
    return scale * src @ R.T + t + noise * rng.normal(size=src.shape), (scale, R, t)


def _cloud(name, seed, n, scale=1.7, offset=0.0, noise=1e-3, B=1, weights=None, estimate_scale=True, flat=None):
    rng = np.random.default_rng(seed)
    src = rng.normal(size=(B, n, 3))
    if flat is not None:
        src[..., 2] *= flat
    src = src + offset
    tgt, truth = zip(*[_moved(rng, src[b], scale if estimate_scale else 1.0, offset, noise) for b in range(B)])
    w = None if weights is None else weights(rng, B, n)
    return {"name": name, "src": src, "tgt": np.stack(tgt), "weights": w, "estimate_scale": estimate_scale, "truth": truth,
            "noise": noise, "valid": True}


def _drop(k):
    def make(rng, B, n):
        w = np.ones((B, n))
        for b in range(B):
            w[b, rng.choice(n, size=k + b * 7, replace=False)] = 0.0
        return w
    return make


def _reflection(seed):
    """Near-planar points whose noise makes the unconstrained least-squares solution a reflection."""
    for s in range(seed, seed + 200):
        c = _cloud("reflection", s, 12, noise=2e-2, flat=1e-3)
        ds = c["src"][0] - c["src"][0].mean(0)
        dtg = c["tgt"][0] - c["tgt"][0].mean(0)
        U, _, Vt = np.linalg.svd(dtg.T @ ds)
        if np.linalg.det(U) * np.linalg.det(Vt) < 0:
            c["seed_used"] = s
            return c
    raise AssertionError("no reflection case found")


def fit_cases():
    cases = [
        _cloud("n3", 11, 3, noise=0.0),
        _cloud("n4_one_masked", 12, 4, noise=0.0, weights=_drop(1)),
        _cloud("n63", 13, 63), _cloud("n64", 14, 64), _cloud("n65", 15, 65), _cloud("n257", 16, 257),
        _cloud("n5000_multi_workgroup", 17, 5000),
        _cloud("b3_masks", 18, 100, B=3, weights=_drop(20)),
        _cloud("float_weights", 19, 80, weights=lambda rng, B, n: rng.uniform(0.0, 2.0, size=(B, n)) * (rng.uniform(size=(B, n)) > 0.2)),
        _cloud("no_scale", 20, 70, estimate_scale=False),
        _cloud("scale_1e-3_offset_1e4", 21, 200, scale=1e-3, offset=1e4, noise=1e-7),
        _cloud("scale_1e3_offset_1e4", 22, 200, scale=1e3, offset=1e4, noise=1e-1),
        _cloud("n5000_offset_1e4", 23, 5000, scale=2.5, offset=1e4, noise=1e-3),
        _reflection(100),
        _cloud("planar", 24, 50, flat=0.0),
    ]
    rng = np.random.default_rng(25)
    line = np.outer(np.linspace(-1, 1, 20), [1.0, 2.0, -0.5]) + [0.3, 0.1, 0.2]
    bad = {"collinear": (line, None), "coincident": (np.tile([[0.5, -1.0, 2.0]], (20, 1)), None),
           "two_points": (rng.normal(size=(20, 3)), np.r_[1.0, 1.0, np.zeros(18)])}
    for name, (src, w) in bad.items():
        cases.append({"name": name, "src": src[None], "tgt": _moved(rng, src, 1.3)[0][None], "weights": None if w is None else w[None],
                      "estimate_scale": True, "valid": False, "noise": 0.0})
    return {c["name"]: c for c in cases}


def robust_scene(seed, B, N, sigma=1e-3, outliers=0.3, scale=2.0):
    """B problems of N correspondences: Gaussian noise sigma on the target, `outliers` of the points replaced by
    uniform draws from the target's box; max_error differs between the problems (5 sigma times 1, 1.1, ...)."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-1, 1, size=(B, N, 3))
    tgt, truth, out = [], [], np.zeros((B, N), bool)
    for b in range(B):
        y, T = _moved(rng, src[b], scale * (1 + 0.5 * b), 0.0, sigma)
        bad = rng.choice(N, size=int(outliers * N), replace=False)
        y[bad] = rng.uniform(y.min(0), y.max(0), size=(len(bad), 3))
        out[b, bad] = True
        tgt.append(y)
        truth.append(T)
    return {"src": src, "tgt": np.stack(tgt), "truth": truth, "outlier": out, "sigma": sigma,
            "max_error": 5 * sigma * (1 + 0.1 * np.arange(B))}


SCORE_TILE = 32            # kTile of csrc/sim3.hip: hypotheses per workgroup of the score pass


def score_case(H, seed=31):
    """B = 2, N = 300, 30 % gross outliers, H hypotheses per problem from 3-point samples (every seventh sample repeats an
    index and is invalid)."""
    sc = robust_scene(seed, 2, 300)
    rng = np.random.default_rng(seed + 1000 + H)
    samples = np.stack([np.stack([rng.choice(300, size=3, replace=False) for _ in range(H)]) for _ in range(2)]).astype(np.int32)
    samples[:, 6::7, 1] = samples[:, 6::7, 0]
    sc["samples"] = samples
    return sc


def ransac_case(seed=41):
    """B = 3, N = 400, H = 128, samples drawn with replacement and every sixteenth made to repeat an index; problem 1
    carries a mask that hides every ninth point; problem 2 draws tight triples only."""
    sc = robust_scene(seed, 3, 400)
    rng = np.random.default_rng(seed + 1)
    sc["samples"] = rng.integers(0, 400, size=(3, 128, 3)).astype(np.int32)
    # problem 2 samples tight triples only (an inlier and its two nearest inliers): every minimal hypothesis extrapolates
    # badly, the winner holds a fraction of the inliers and the LO rounds have work to do
    good = np.nonzero(~sc["outlier"][2])[0]
    for h in range(128):
        c = sc["src"][2][good[h % 8]]
        sc["samples"][2, h] = rng.permutation(good[np.argsort(np.linalg.norm(sc["src"][2][good] - c, axis=1))[:3]])
    sc["samples"][:, 5::16, 2] = sc["samples"][:, 5::16, 0]          # samples that repeat an index
    mask = np.ones((3, 400), bool)
    mask[1, ::9] = False
    sc["mask"] = mask
    return sc


def pose_set(S, seed, rot_noise=0.05, trans_noise=0.05):
    """(pred, gt) world-to-camera (S,3,4): gt random, pred = gt disturbed."""
    rng = np.random.default_rng(seed)
    gt, pred = np.zeros((S, 3, 4)), np.zeros((S, 3, 4))
    for i in range(S):
        R, c = random_rotation(rng), rng.normal(size=3) * 3
        w = rng.normal(size=3) * rot_noise
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        th = np.linalg.norm(w)
        dR = np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th ** 2) * K @ K if th > 0 else np.eye(3)
        gt[i, :, :3], gt[i, :, 3] = R, -R @ c
        pred[i, :, :3], pred[i, :, 3] = dR @ R, -(dR @ R) @ (c + trans_noise * rng.normal(size=3))
    return pred, gt


def same_centre_poses(poses):
    """A copy whose cameras 0 and 1 are both [I | t0]: equal centres and a relative translation that is exactly zero."""
    out = np.array(poses)
    out[0, :, :3] = out[1, :, :3] = np.eye(3)
    out[1, :, 3] = out[0, :, 3]
    return out


def recovery(T, truth, src, inliers, sigma):
    """[(error, bound)] of an estimate from n inliers with isotropic target noise sigma against the known transform, each
    bound three standard deviations of the least-squares estimate (r = rms radius of the inliers about their centroid):
    the centroid's image per axis sigma / sqrt(n); the relative scale sigma / (s r sqrt(n)); the rotation angle, three
    axes of sigma / (s r sqrt(2 n / 3)) each."""
    s, R, t = (np.asarray(x, np.float64) for x in T)
    s0, R0, t0 = truth
    pts = np.asarray(src)[np.asarray(inliers, bool)]
    n, mu = len(pts), pts.mean(0)
    r = np.sqrt(((pts - mu) ** 2).sum(1).mean())
    centre = np.abs((s * R @ mu + t) - (s0 * R0 @ mu + t0)).max()
    angle = np.arccos(np.clip((np.trace(R0.T @ R) - 1) / 2, -1, 1))
    return [(centre, 3 * sigma / np.sqrt(n)), (abs(s - s0) / s0, 3 * sigma / (s0 * r * np.sqrt(n))),
            (angle, 3 * np.sqrt(3) * sigma / (s0 * r * np.sqrt(2 * n / 3)))]
