"""EPnP and its use as the local optimisation of the P3P RANSAC: scenes, an independent CPU solver and the restated LO loop
(a helper module, not a test file).

  scene / lo_scene            seeded generators
  epnp                        EPnP in numpy float64, following the steps of the reference's ``efficient_pnp``
                              (vggsfm/two_view_geo/perspective_n_points.py:36-437) with numpy's own inverse, eigh, pinv and
                              svd; it returns ALL candidates (4, or 1 with skip_quadratic), not only the winner
  wmean, corresponding_points_alignment
                              stand-ins for the two PyTorch3D names the reference's module imports (a weighted mean, and
                              Umeyama with scale), in torch, used only where the reference's own function is run
  score, local_optimisation   the support rule of vgg_p3p_ransac and the LO loop of vggp_epnp_lo in numpy
  GOLDEN_CASES, golden_inputs the cases of tests/golden/pnp_epnp.npz (scripts/make_golden_pnp.py writes the file)
"""
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_epnp.npz")
EPS = 1e-9
LO_MIN_INLIERS = 6

# The CPU solver (kernel vectors signed like the reference's) against the reference's own function over all golden cases,
# measured on the CPU: R 2.5e-12 (Frobenius, the N = 5 case), T 1.1e-12 and x_cam 9.4e-13 relative, err_2d 1.2e-10 of
# max(err_2d, ERR_SCALE) (1.2e-13 absolute, N = 5).  The bound is one decade above the largest.
YARDSTICK_BOUND = 1.2e-9
# err_2d is a mean distance on the normalised image plane; on exact data it is rounding noise (1e-15), so a difference of
# two err_2d is taken relative to max(err_2d, ERR_SCALE), ERR_SCALE = the noise of the noisy cases
ERR_SCALE = 1e-3
# The CPU solver against the true pose on the noise-free golden cases: R 1.7e-12 (N = 5), T 1.7e-13 relative; one decade above
TRUE_POSE_BOUND = 1.8e-11


# --- scenes --------------------------------------------------------------------------------------------------------------
def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene(rng, n, noise=0.0, distance=4.0, planar=False):
    """n points in a cube of side 2 about `distance` from the camera.  Returns x (n,3), y (n,2) = Proj(x R + T) + noise,
    R (3,3), T (3,) in the reference's row-vector convention."""
    x = rng.uniform(-1.0, 1.0, (n, 3))
    if planar:
        x[:, 2] = 0.0
    R = random_rotation(rng)
    T = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), distance * rng.uniform(0.9, 1.1)])
    xc = x @ R + T
    y = xc[:, :2] / xc[:, 2:] + noise * rng.normal(size=(n, 2))
    return x, y, R, T


# name -> (N, noise, what); B = 7 problems each
GOLDEN_B = 7
GOLDEN_CASES = {
    "clean_5": (5, 0.0, None), "clean_6": (6, 0.0, None), "clean_8": (8, 0.0, None), "clean_12": (12, 0.0, None),
    "clean_65": (65, 0.0, None), "clean_257": (257, 0.0, None),
    "noisy_6": (6, 1e-3, None), "noisy_12": (12, 1e-3, None), "noisy_65": (65, 1e-3, None), "noisy_257": (257, 1e-3, None),
    "masked_6_of_40": (40, 0.0, "six"), "masked_half": (40, 0.0, "half"), "far": (12, 0.0, "far"),
    "skip_quadratic": (12, 0.0, "skip"),
}
NOISE_FREE = [k for k, (_, noise, what) in GOLDEN_CASES.items() if noise == 0.0]
GOLDEN_SEED = 1701


def golden_inputs():
    """name -> dict(x (B,N,3), y (B,N,2), masks (B,N) bool or None, skip bool, R_true (B,3,3), T_true (B,3))"""
    out = {}
    for i, (name, (n, noise, what)) in enumerate(GOLDEN_CASES.items()):
        rng = np.random.default_rng(GOLDEN_SEED + i)
        xs, ys, Rs, Ts = zip(*(scene(rng, n, noise, distance=200.0 if what == "far" else 4.0) for _ in range(GOLDEN_B)))
        x, y = np.stack(xs), np.stack(ys)
        masks = None
        if what in ("six", "half"):
            masks = np.zeros((GOLDEN_B, n), bool)
            for b in range(GOLDEN_B):
                masks[b, rng.permutation(n)[:6 if what == "six" else n // 2]] = True
            if what == "six":                       # garbage in the masked-out slots
                x, y = x.copy(), y.copy()
                x[~masks] = 7.0
                y[~masks] = 7.0
        out[name] = dict(x=x, y=y, masks=masks, skip=what == "skip", R_true=np.stack(Rs), T_true=np.stack(Ts))
    return out


def load_golden():
    g = np.load(GOLDEN)
    out = {}
    for name in GOLDEN_CASES:
        c = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}
        c["masks"] = c["masks"] if "masks" in c else None
        c["skip"] = bool(c["skip"])
        out[name] = c
    return out


# --- the CPU solver --------------------------------------------------------------------------------------------------------
_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def _wmean_np(v, w):
    return (v * w[:, None]).sum(0) / max(w.sum(), EPS)


def _umeyama(xw, xc, w):
    """R, T, s with xc ~ s xw R + T over the points weighted by w (0/1) -- Umeyama 1991 as PyTorch3D states it"""
    xmu, ymu = _wmean_np(xw, w), _wmean_np(xc, w)
    a, b = (xw - xmu) * w[:, None], (xc - ymu) * w[:, None]
    tw = max(w.sum(), EPS)
    cov = a.T @ b / tw
    U, S, Vt = np.linalg.svd(cov)
    E = np.ones(3)
    E[2] = np.linalg.det(U @ Vt)
    R = (U * E) @ Vt
    s = (E * S).sum() / max((a * a).sum() / tw, EPS)
    return R, ymu - s * (xmu @ R), s


def _null_space_coords(case, L, rhs):
    cols = {1: [0, 4, 5, 6], 2: [0, 4, 1], 3: [0, 4, 1, 5, 7]}[case]
    b = np.linalg.pinv(L[:, cols]) @ rhs
    sign = lambda t: 1.0 if t >= 0 else -1.0
    if case == 1:
        b = b * sign(b[0])
        return b / max(np.sqrt(b[0]), EPS)
    c0 = np.sqrt(abs(b[0])) * sign(b[1])
    c1 = np.sqrt(abs(b[2])) * float((b[0] >= 0) == (b[2] >= 0))
    if case == 2:
        return np.array([c0, c1, 0.0, 0.0])
    return np.array([c0, c1, b[3] / max(c0, EPS), 0.0])


def epnp(x, y, mask=None, skip_quadratic=False, kernel_like=None):
    """One problem: x (N,3), y (N,2), mask (N,) bool or None.  Returns a list of candidates (dict R, T, x_cam, err_2d,
    err_3d), candidate 0 = the kernel vector alone, 1..3 = cases 1..3, and the index of the first minimum of err_2d.  Rows
    that are masked out are removed before anything is computed (x_cam has zeros there).

    The sign of a kernel vector is the eigensolver's business, and case 3 depends on it: it divides by clamp(coord_0, 1e-9)
    and coord_0 carries the sign of B12, so the case gives a pose only when kernel vectors 0 and 1 come out with B12 > 0.
    Here, as on the device, every kernel vector has its component of largest magnitude (the first such) positive.  With
    `kernel_like` (12,4) each vector instead takes the sign that gives it a positive scalar product with that column: this
    is how the reference's result, made with the signs of its own eigensolver, is reproduced."""
    n = len(x)
    keep = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    xs, ys = x[keep], y[keep]
    w = np.ones(len(xs))
    mean = _wmean_np(xs, w)
    c_world = np.vstack([np.eye(3), np.zeros((1, 3))]) + mean
    alphas = np.hstack([xs, np.ones((len(xs), 1))]) @ np.linalg.inv(np.hstack([c_world, np.ones((4, 1))]))
    M = np.zeros((2 * len(xs), 12))
    for j in range(4):
        M[0::2, 3 * j] = alphas[:, j]
        M[0::2, 3 * j + 2] = -alphas[:, j] * ys[:, 0]
        M[1::2, 3 * j + 1] = alphas[:, j]
        M[1::2, 3 * j + 2] = -alphas[:, j] * ys[:, 1]
    _, vecs = np.linalg.eigh(M.T @ M)
    vecs = vecs[:, :4].copy()
    for k in range(4):
        if kernel_like is None:
            flip = vecs[np.argmax(np.abs(vecs[:, k])), k] < 0
        else:
            flip = vecs[:, k] @ kernel_like[:, k] < 0
        vecs[:, k] = -vecs[:, k] if flip else vecs[:, k]
    kernel = vecs.reshape(4, 3, 4)                               # (control point, coordinate, kernel vector)
    dv = np.stack([kernel[l] - kernel[r] for l, r in _PAIRS])    # (6, 3, 4)
    L = np.concatenate([(dv ** 2).sum(1), np.stack([2.0 * (dv[:, :, i] * dv[:, :, j]).sum(1) for i, j in _PAIRS], 1)], 1)
    rhs = np.array([((c_world[l] - c_world[r]) ** 2).sum() for l, r in _PAIRS])
    betas = [np.array([1.0, 0, 0, 0])] + ([] if skip_quadratic else [_null_space_coords(c, L, rhs) for c in (1, 2, 3)])
    out = []
    for beta in betas:
        with np.errstate(all="ignore"):
            c_cam = kernel @ beta
            xc = alphas @ c_cam
            if _wmean_np(xc[:, 2:], w)[0] < 0:
                xc = -xc
            R, T, s = _umeyama(xs, xc, w)
            s = max(s, EPS)
            xc, T = xc / s, T / s
            xr = xs @ R + T
            proj = xr[:, :2] / np.maximum(xr[:, 2:], EPS)
            e2 = np.sqrt(((ys - proj) ** 2).sum(1)).mean()
            e3 = ((xr - xc) ** 2).sum(1).mean()
        full = np.zeros((n, 3))
        full[keep] = xc
        out.append(dict(R=R, T=T, x_cam=full, err_2d=e2, err_3d=e3))
    return out, int(np.argmin([c["err_2d"] for c in out]))


# --- stand-ins for the PyTorch3D names of the reference's module (torch; only for running the reference's function) ------------
def wmean(x, weight=None, dim=-2, keepdim=True, eps=EPS):
    if weight is None:
        return x.mean(dim=dim, keepdim=keepdim)
    return (x * weight[..., None]).sum(dim=dim, keepdim=keepdim) / weight[..., None].sum(dim=dim, keepdim=keepdim).clamp(eps)


def corresponding_points_alignment(X, Y, weights=None, estimate_scale=False, allow_reflection=False, eps=EPS):
    import torch
    b, n, dim = X.shape
    xmu, ymu = wmean(X, weights, eps=eps), wmean(Y, weights, eps=eps)
    xc, yc = X - xmu, Y - ymu
    total = torch.full((b,), float(max(n, 1)), dtype=X.dtype)
    if weights is not None:
        xc, yc = xc * weights[:, :, None], yc * weights[:, :, None]
        total = weights.sum(1).clamp(eps)
    cov = torch.bmm(xc.transpose(2, 1), yc) / total[:, None, None]
    U, S, Vh = torch.linalg.svd(cov)
    E = torch.eye(dim, dtype=X.dtype)[None].repeat(b, 1, 1)
    if not allow_reflection:
        E[:, -1, -1] = torch.det(torch.bmm(U, Vh))
    R = torch.bmm(torch.bmm(U, E), Vh)
    if estimate_scale:
        s = (torch.diagonal(E, dim1=1, dim2=2) * S).sum(1) / ((xc * xc).sum((1, 2)) / total).clamp(eps)
    else:
        s = torch.ones(b, dtype=X.dtype)
    T = ymu[:, 0, :] - s[:, None] * torch.bmm(xmu, R)[:, 0, :]
    return R, T, s


def pytorch3d_stand_ins():
    """(oputil, points_alignment) to set on the reference's module"""
    return SimpleNamespace(wmean=wmean), SimpleNamespace(corresponding_points_alignment=corresponding_points_alignment)


# --- support and the local optimisation -------------------------------------------------------------------------------------
def residuals(pose, xn, X):
    """squared residuals on the normalised plane and the depths: pose (3,4) = [R|t], xn (P,2), X (P,3)"""
    pc = X @ pose[:, :3].T + pose[:, 3]
    front = pc[:, 2] > 1e-12
    z = np.where(front, pc[:, 2], 1.0)
    return ((pc[:, :2] / z[:, None] - xn) ** 2).sum(1), front


def score(pose, xn, X, cand, thr_sq):
    """(count, residual sum, mask) of pose under the support rule of vgg_p3p_ransac"""
    r, front = residuals(pose, xn, X)
    inl = front & (r <= thr_sq) & (np.ones(len(X), bool) if cand is None else cand)
    return int(inl.sum()), float(r[inl].sum()), inl


def local_optimisation(pose, num, xn, X, cand, thr_sq, max_rounds):
    """The loop of vggp_epnp_lo for one frame.  Returns (pose, count, residual sum, mask, history of (count, sum))."""
    if num <= 0:
        return pose, num, None, None, []
    cnt, rs, mask = score(pose, xn, X, cand, thr_sq)
    history = [(cnt, rs)]
    for _ in range(max_rounds):
        if cnt < LO_MIN_INLIERS:
            break
        cands, best = epnp(X, xn, mask)
        c = cands[best]
        if not all(np.isfinite(k[f]).all() for k in cands for f in ("R", "T", "err_2d", "err_3d")):
            break
        new = np.hstack([c["R"].T, c["T"][:, None]])
        c2, s2, m2 = score(new, xn, X, cand, thr_sq)
        if not (c2 > cnt or (c2 == cnt and s2 < rs)):
            break
        pose, cnt, rs, mask = new, c2, s2, m2
        history.append((cnt, rs))
    return pose, cnt, rs, mask, history


LO_SEED = 11


def lo_scene(seed=LO_SEED, F=3, P=300, outliers=0.3, thr=0.01):
    """F frames looking at the same P points: inlier noise thr / 5 per coordinate (capped at thr / 2 so that every true inlier
    stays one), `outliers` of the matches moved by more than 20 thr; frame 2's candidate mask drops every third point.
    Returns dict(X (P,3), xn (F,P,2), cand (F,P) bool, thr_sq (F,), pose_true (F,3,4), outlier (F,P) bool)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (P, 3))
    xn, poses, outl = np.empty((F, P, 2)), np.empty((F, 3, 4)), np.zeros((F, P), bool)
    for f in range(F):
        R = random_rotation(rng)
        T = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 4.0 * rng.uniform(0.9, 1.1)])
        pc = X @ R + T
        xn[f] = pc[:, :2] / pc[:, 2:] + np.clip(rng.normal(size=(P, 2)) * thr / 5, -thr / 2, thr / 2)
        bad = rng.permutation(P)[:int(outliers * P)]
        ang = rng.uniform(0, 2 * np.pi, len(bad))
        xn[f, bad] += (rng.uniform(25, 60, len(bad)) * thr)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
        outl[f, bad] = True
        poses[f] = np.hstack([R.T, T[:, None]])
    cand = np.ones((F, P), bool)
    if F > 2:
        cand[2, ::3] = False
    return dict(X=X, xn=xn, cand=cand, thr_sq=np.full(F, thr * thr), pose_true=poses, outlier=outl)


def p3p_seed_poses(sc, H=16, seed=5):
    """(F,H,3) int32 minimal samples for vgg_p3p_ransac on a lo_scene, drawn from each frame's candidates"""
    rng = np.random.default_rng(seed)
    F, P = sc["cand"].shape
    out = np.empty((F, H, 3), np.int32)
    for f in range(F):
        idx = np.nonzero(sc["cand"][f])[0]
        for h in range(H):
            out[f, h] = rng.choice(idx, 3, replace=False)
    return out


def p3p_incoming_cpu(sc, samples):
    """The incoming poses of the LO on the CPU: oracle/p3p.py (operation by operation what vgg_p3p_ransac computes) on the
    recorded samples.  Returns (pose (F,3,4), num_inliers (F,))."""
    from oracle import p3p as OP
    F = len(sc["xn"])
    res = [OP.absolute_pose_ransac(sc["xn"][f], sc["X"], sc["cand"][f], samples[f], sc["thr_sq"][f]) for f in range(F)]
    return np.stack([r["pose"] for r in res]), np.array([r["num_inliers"] for r in res])


def near_threshold(pose, xn, X, cand, thr_sq, rel=1e-9):
    """candidates whose residual under pose lies within `rel` relative of the threshold: what a comparison has to leave out"""
    r, _ = residuals(pose, xn, X)
    return (np.abs(r - thr_sq) <= rel * thr_sq) & cand
