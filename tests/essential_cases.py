"""Shared by the essential-matrix tests and scripts/make_golden_essential.py: an independent CPU 5-point solver (numpy
float64, Stewenius' action matrix -- not the route of csrc/essential.hip, which eliminates to a degree-10 polynomial),
synthetic two-view scenes, set comparison up to sign, and the golden files' names and caps."""
import glob
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

FLOW_CASES = ("flow_equal", "flow_mixed")
ALL_FILES = ("solver",) + FLOW_CASES
CAP = 0.02                 # no file leaves out more than this share of its samples or matches
DISTINCT = 1e-6            # candidates further apart than this (Frobenius, up to sign) are different candidates
MARGIN = 1e-3              # relative: mean-residual margin of the winner, and the band around the threshold
JITTER, STABLE = 1e-13, 1e-7

# Largest deviation (Frobenius, up to sign) of a device candidate from the CPU solver's on the admitted samples of
# essential_solver.npz, measured on an MI355X: DESIGN.md section 16.  The bound is one decade above it.
SOLVER_MEASURED = 2.934e-10
SOLVER_BOUND = 10 * SOLVER_MEASURED
FLOW_BOUND = 10 * SOLVER_BOUND          # local optimisation adds a 9x9 eigen-solve
CONSTRAINT_BOUND = 1e-8                 # |p2^T E p1|, |det E|, ||2 E E^T E - tr(E E^T) E|| at ||E|| = 1
# Largest angular error of the recovered pose in the production configuration (radians) measured on an MI355X: rotation
# 3.5e-15, translation direction 1.9e-14; the bound is one decade above the larger
POSE_MEASURED = 1.871e-14
POSE_BOUND = 10 * POSE_MEASURED


def files():
    return sorted(glob.glob(os.path.join(GOLDEN, "essential_*.npz")))


def load(name):
    with np.load(os.path.join(GOLDEN, f"essential_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


# --- polynomials in (x, y, z) of total degree <= 3 as (4,4,4) coefficient arrays ---------------------------------------
def _pmul(p, q):
    r = np.zeros((4, 4, 4))
    for a, b, c in zip(*np.nonzero(p)):
        r[a:, b:, c:] += p[a, b, c] * q[:4 - a, :4 - b, :4 - c]
    return r


# cubic monomials first, then the basis of the quotient ring
_MONOMIALS = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
              (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def null_space(points1, points2, weights=None):
    """(4,9) orthonormal basis of the null space of the epipolar rows: the last right singular vectors of X itself."""
    x1, y1, x2, y2 = points1[:, 0], points1[:, 1], points2[:, 0], points2[:, 1]
    X = np.stack([x1 * x2, x1 * y2, x1, y1 * x2, y1 * y2, y1, x2, y2, np.ones_like(x1)], 1)
    if weights is not None:
        X = X * weights[:, None]
    if X.shape[0] < 9:
        X = np.concatenate([X, np.zeros((9 - X.shape[0], 9))])
    return np.linalg.svd(X)[2][-4:]


def solve_null_space(basis):
    """All real E = x N0 + y N1 + z N2 + N3 with det E = 0 and 2 E E^T E - tr(E E^T) E = 0 -> (k,3,3), unit Frobenius
    norm, laid out so that p2^T E p1 = 0 for rows [x1 x2, x1 y2, x1, y1 x2, ...]."""
    Ep = np.zeros((3, 3, 4, 4, 4))
    Ep[:, :, 1, 0, 0], Ep[:, :, 0, 1, 0], Ep[:, :, 0, 0, 1], Ep[:, :, 0, 0, 0] = (basis[k].reshape(3, 3) for k in range(4))
    det = (_pmul(_pmul(Ep[0, 1], Ep[1, 2]) - _pmul(Ep[0, 2], Ep[1, 1]), Ep[2, 0])
           + _pmul(_pmul(Ep[0, 2], Ep[1, 0]) - _pmul(Ep[0, 0], Ep[1, 2]), Ep[2, 1])
           + _pmul(_pmul(Ep[0, 0], Ep[1, 1]) - _pmul(Ep[0, 1], Ep[1, 0]), Ep[2, 2]))
    EEt = [[sum(_pmul(Ep[i, m], Ep[j, m]) for m in range(3)) for j in range(3)] for i in range(3)]
    tr = EEt[0][0] + EEt[1][1] + EEt[2][2]
    cons = [det]
    for i in range(3):
        for j in range(3):
            cons.append(sum(_pmul(2 * EEt[i][k] - (tr if i == k else 0), Ep[k, j]) for k in range(3)))
    M = np.array([[c[m] for m in _MONOMIALS] for c in cons])
    try:
        Bm = np.linalg.solve(M[:, :10], M[:, 10:])
    except np.linalg.LinAlgError:
        return np.zeros((0, 3, 3))
    if not np.isfinite(Bm).all():
        return np.zeros((0, 3, 3))
    # multiplication by x in the basis [x^2 xy xz y^2 yz z^2 x y z 1]: the first six products are cubic monomials
    A = np.zeros((10, 10))
    A[0], A[1], A[2], A[3], A[4], A[5] = -Bm[0], -Bm[1], -Bm[2], -Bm[3], -Bm[4], -Bm[5]
    A[6, 0] = A[7, 1] = A[8, 2] = A[9, 6] = 1.0
    w, V = np.linalg.eig(A)
    out = []
    for k in np.nonzero(np.isreal(w))[0]:
        v = V[:, k].real
        x, y, z = v[6] / v[9], v[7] / v[9], v[8] / v[9]
        e = x * basis[0] + y * basis[1] + z * basis[2] + basis[3]
        if np.isfinite(e).all() and np.linalg.norm(e) > 0:
            out.append((e / np.linalg.norm(e)).reshape(3, 3).T)
    return np.array(out).reshape(-1, 3, 3)


def five_point(points1, points2, weights=None):
    """points (n >= 5, 2) normalised [, weights (n,) on the rows] -> (k,3,3) real solutions."""
    return solve_null_space(null_space(np.asarray(points1, np.float64), np.asarray(points2, np.float64), weights))


# --- comparison up to sign -------------------------------------------------------------------------------------------------
def distance(E, F):
    """Frobenius distance up to sign of (...,3,3) arrays (broadcast)."""
    return np.minimum(np.linalg.norm(E - F, axis=(-2, -1)), np.linalg.norm(E + F, axis=(-2, -1)))


def set_deviation(A, B):
    """Largest distance from a member of one (k,3,3) set to the nearest member of the other (inf for unequal sizes)."""
    if len(A) != len(B):
        return np.inf
    if len(A) == 0:
        return 0.0
    D = distance(A[:, None], B[None])
    return float(max(D.min(1).max(), D.min(0).max()))


def constraint_residuals(E, p1, p2):
    """max |p2^T E p1| over the given points, |det E|, ||2 E E^T E - tr(E E^T) E|| of one 3x3 E."""
    h1 = np.concatenate([p1, np.ones((len(p1), 1))], 1)
    h2 = np.concatenate([p2, np.ones((len(p2), 1))], 1)
    EEt = E @ E.T
    return (float(np.abs(np.einsum("ni,ij,nj->n", h2, E, h1)).max()), float(abs(np.linalg.det(E))),
            float(np.linalg.norm(2 * EEt @ E - np.trace(EEt) * E)))


def sampson_sq(E, p1, p2):
    """float64 squared Sampson distance of (N,2) points under (...,3,3) matrices -> (...,N)."""
    h1 = np.concatenate([p1, np.ones((len(p1), 1))], 1)
    h2 = np.concatenate([p2, np.ones((len(p2), 1))], 1)
    l = np.einsum("...ij,nj->...ni", E, h1)
    m = np.einsum("...ji,nj->...ni", E, h2)
    num = np.einsum("...ni,ni->...n", l, h2) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        r = num / (l[..., 0] ** 2 + l[..., 1] ** 2 + m[..., 0] ** 2 + m[..., 1] ** 2)
    return np.where(np.isfinite(r), r, 1e6)


# --- scenes --------------------------------------------------------------------------------------------------------------------
def rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def two_view_scene(rng, N, focal, principal, noise=0.0, outliers=0.0, outlier_clearance=0.0):
    """One pair: camera 1 = [I | 0], camera 2 = [R | t].  focal, principal (4,) as build_default_kmat lays them out.
    Returns pixels1, pixels2 (N,2), R, t (unit), inlier flags (N,); the first matches are the outliers.  With
    outlier_clearance (pixels) an outlier is drawn again until its Sampson distance to the true E exceeds that."""
    R = rodrigues(rng.uniform(-0.25, 0.25, 3) + 1e-3)
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    X = np.stack([rng.uniform(-2, 2, N), rng.uniform(-2, 2, N), rng.uniform(4, 9, N)], 1)
    Y = X @ R.T + t
    x1, x2 = X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]
    px1 = x1 * focal[:2] + principal[:2] + noise * rng.normal(size=(N, 2))
    px2 = x2 * focal[2:] + principal[2:] + noise * rng.normal(size=(N, 2))
    n_out = int(round(outliers * N))
    px2[:n_out] = principal[2:] + focal[2:] * rng.uniform(-0.5, 0.5, (n_out, 2))
    if outlier_clearance > 0:
        E, limit = true_essential(R, t), (outlier_clearance / np.mean(focal)) ** 2
        for n in range(n_out):
            while sampson_sq(E, *normalise(px1[n:n + 1], px2[n:n + 1], focal, principal))[0] <= limit:
                px2[n] = principal[2:] + focal[2:] * rng.uniform(-0.5, 0.5, 2)
    inl = np.ones(N, bool)
    inl[:n_out] = False
    return px1, px2, R, t, inl


def true_essential(R, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return E / np.linalg.norm(E)


def normalise(px1, px2, focal, principal):
    return (px1 - principal[:2]) / focal[:2], (px2 - principal[2:]) / focal[2:]
