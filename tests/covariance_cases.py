"""Shared by tests/test_covariance_reference.py (CPU) and tests/test_gpu_covariance.py: a long-double reference of the bundle
adjustment covariance (include/vggsfm_amd_covariance.h) on cases of tests/ba_system_cases.py, at their perturbed start point.

The reference starts where that module's does -- `compile_case` / `host_arrays` and oracle/ba_autograd's `_Problem.blocks`
(torch.func.jacrev Jacobian blocks F, E with the sqrt(rho') correction, constant and unobserved columns zero) -- and is dense
algebra in numpy behind them, UNSCALED and UNDAMPED, by two routes:

  (A) `dense_route`: H = J^T J over all columns -- cameras, intrinsics and points together, no Schur complement --, unit
      diagonal on the inactive ones, inverted by the row-operation Cholesky of ba_system_cases (here with the identity as its
      right-hand sides), inactive rows and columns zeroed.  Cases small enough: DENSE_CASES.
  (B) `schur_route`: S = H_cc - sum_p W_p V_p^-1 W_p^T, Sigma_cc = S^-1 the same way, Sigma_pp = V_p^-1 + G Sigma_uu G^T with
      G = V_p^-1 W_p^T over the point's columns u (3 x 3 inverse by adjugate).  Every case of CASES.

Measure, per block type (pose 6 x 6 per camera, intrinsics kd x kd per block, pose-intrinsics 6 x kd per camera, points 3 x 3):
max |delta_ij| / sqrt(Sigma_ii Sigma_jj) with the REFERENCE's variances, over the entries whose two variances are positive.
`reference(name)` = route (B) in numpy.longdouble, `dev` = the deviation of its float64 evaluation from that, and the GPU
tests' bounds by the rule of ba_system_cases: max(FLOOR_STEP = 1e-11, 100 x dev).

Measured on x86-64 (80-bit long double), tests/test_covariance_reference.py prints them --
  (A) against (B), long double:   a  pose 4.6e-13  intrinsics 4.6e-13  pose_intrinsics 4.6e-13  points 4.6e-13
                                  c  pose 7.0e-13  intrinsics 6.8e-15  pose_intrinsics 3.2e-14  points 7.0e-13
  (2^-11 of the float64 deviations below, as two long-double evaluations should differ)
  float64 (B) against long double (B):
    case     pose      intrinsics  pose_intrinsics  points
    a        1.3e-09   1.3e-09     1.3e-09          1.3e-09
    c        2.0e-09   6.2e-11     3.2e-10          2.0e-09
    d        2.2e-09   2.4e-10     1.8e-10          2.2e-09
    e        2.3e-09   1.5e-11     8.9e-11          2.4e-09
    h        7.6e-09   8.3e-11     8.6e-10          7.7e-09
    i_none   1.3e-11   -           -                8.8e-12
    i_extra  4.1e-10   7.0e-12     5.5e-11          4.2e-10
    j        9.8e-14   -           -                3.4e-14
    g        3.0e-08   4.0e-11     1.0e-09          3.0e-08
    l_env    2.2e-05   4.6e-09     2.6e-07          2.2e-05
The deviations are those of an inverse: they grow with the condition of the reduced system, which at the perturbed start point
with the minimal gauge (seven fixed columns) reaches 7e11 on l_env (2e10 with its diagonal scaled to one); where the gauge
is wide (j: five constant poses and 150 constant points) float64 is at 1e-13."""
import time
from types import SimpleNamespace

import numpy as np

from oracle import ba_autograd as AG
from tests import ba_system_cases as SC

LD = np.longdouble
CASES = ("a", "c", "d", "e", "h", "i_none", "i_extra", "j", "g", "l_env")     # (i_extra: kd = 1 from k alone, the only_k path)
DENSE_CASES = ("a", "c")
BLOCKS = ("pose", "intrinsics", "pose_intrinsics", "points")


def cholesky_inverse(A):
    """A^-1 in A's number type (lower triangle read): ba_system_cases.cholesky_solve's right-looking factorisation by row
    operations, then L^-1 by forward substitution of the identity (row j of it ends at column j) and A^-1 = L^-T L^-1."""
    n = len(A)
    L = np.tril(A).copy()
    for j in range(n):
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
        if j + 1 < n:
            v = L[j + 1:, j]
            L[j + 1:, j + 1:] -= np.tril(np.outer(v, v))
    X = np.eye(n, dtype=A.dtype)
    for j in range(n):
        X[j, :j + 1] /= L[j, j]
        X[j + 1:, :j + 1] -= np.outer(L[j + 1:, j], X[j, :j + 1])
    out = np.zeros_like(X)                                       # X^T X, 32 rows of the triangular X at a time
    for r0 in range(0, n, 32):
        B = X[r0:r0 + 32, :min(n, r0 + 32)]
        out[:B.shape[1], :B.shape[1]] += B.T @ B
    return out


def _masked_inverse(H, act):
    A = H.copy()
    ina = np.nonzero(~act)[0]
    A[ina, :] = 0
    A[:, ina] = 0
    A[ina, ina] = 1
    Sigma = cholesky_inverse(A)
    Sigma[ina, :] = 0
    Sigma[:, ina] = 0
    return Sigma


def _cut(pb, a, Sigma_cc, Sigma_pp):
    """The blocks the device entry returns, from the reduced covariance and the points' blocks."""
    C, NI, kd = pb.C, pb.NI, pb.kd
    pose = np.stack([Sigma_cc[6 * c:6 * c + 6, 6 * c:6 * c + 6] for c in range(C)])
    io = lambda b: 6 * C + kd * b
    intr = np.stack([Sigma_cc[io(b):io(b) + kd, io(b):io(b) + kd] for b in range(NI)])
    pi = np.stack([Sigma_cc[6 * c:6 * c + 6, io(a.cam_intr[c]):io(a.cam_intr[c]) + kd] for c in range(C)])
    return SimpleNamespace(reduced=Sigma_cc, pose=pose, intrinsics=intr, pose_intrinsics=pi, points=Sigma_pp)


def schur_route(a, pb, blocks, T):
    """Route (B) in the number type T."""
    _, _, F, E, cols = blocks
    F, E = F.astype(T), E.astype(T)
    P, nr = pb.P, pb.n_red
    pt = pb.obs_pt
    H = np.zeros((nr, nr), T)
    np.add.at(H, (cols[:, :, None], cols[:, None, :]), np.einsum("oki,okj->oij", F, F))
    V = np.zeros((P, 3, 3), T)
    np.add.at(V, pt, np.einsum("oki,okj->oij", E, E))
    pt_active = pb.active[nr::3]
    V[~pt_active] = np.eye(3, dtype=T)                          # (not used: keeps the adjugate finite)
    Vi = SC._inv3(V)
    W = np.einsum("oki,okj->oij", F, E)                          # (O, BD, 3)
    row_ptr = a.row_ptr.astype(np.int64)
    S = H.copy()
    per_point = {}
    for p in np.nonzero(pt_active)[0]:
        o0, o1 = row_ptr[p], row_ptr[p + 1]
        u, inv = np.unique(cols[o0:o1].ravel(), return_inverse=True)
        Wp = np.zeros((len(u), 3), T)
        np.add.at(Wp, inv.ravel(), W[o0:o1].reshape(-1, 3))
        WV = Wp @ Vi[p]
        S[np.ix_(u, u)] -= WV @ Wp.T
        per_point[p] = (u, WV)                                   # WV = G^T
    Sigma_cc = _masked_inverse(S, pb.active[:nr])
    Sigma_pp = np.zeros((P, 3, 3), T)
    for p, (u, GT) in per_point.items():
        Sigma_pp[p] = Vi[p] + GT.T @ Sigma_cc[np.ix_(u, u)] @ GT
    return _cut(pb, a, Sigma_cc, Sigma_pp)


def dense_route(a, pb, blocks, T):
    """Route (A) in the number type T: one matrix over every column, no elimination."""
    _, _, F, E, cols = blocks
    F, E = F.astype(T), E.astype(T)
    nr, n = pb.n_red, pb.n
    pcols = nr + 3 * pb.obs_pt[:, None] + np.arange(3)[None]
    allc = np.concatenate([cols, pcols], 1)
    J = np.concatenate([F, E], 2)                                # (O, 2, BD + 3)
    H = np.zeros((n, n), T)
    np.add.at(H, (allc[:, :, None], allc[:, None, :]), np.einsum("oki,okj->oij", J, J))
    Sigma = _masked_inverse(H, pb.active)
    Sigma_pp = np.stack([Sigma[nr + 3 * p:nr + 3 * p + 3, nr + 3 * p:nr + 3 * p + 3] for p in range(pb.P)])
    return _cut(pb, a, Sigma[:nr, :nr], Sigma_pp)


def block_error(got, ref, var_rows, var_cols):
    """max |got - ref|_ij / sqrt(var_rows_i var_cols_j) over a stack of blocks (B, r, c), entries with both variances > 0
    (variances: the REFERENCE's, (B, r) and (B, c)); and whether `got` is exactly zero everywhere else."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref)
    if ref.size == 0:
        return 0.0, True
    vr, vc = np.asarray(var_rows, np.float64), np.asarray(var_cols, np.float64)
    on = (vr[:, :, None] > 0) & (vc[:, None, :] > 0)
    scale = np.sqrt(np.where(on, vr[:, :, None] * vc[:, None, :], 1.0))
    err = np.abs(np.asarray(got - ref, np.float64)) / scale
    return (float(err[on].max()) if on.any() else 0.0), bool((got[~on] == 0).all())


def errors(got, ref):
    """{block type: (error, zeros exact)} of `got` (anything with the members pose, intrinsics, pose_intrinsics, points; None
    = not compared) against the reference's blocks."""
    d = lambda x: np.diagonal(np.asarray(x, np.float64), axis1=1, axis2=2)
    vp, vi, vx = d(ref.pose), d(ref.intrinsics), d(ref.points)
    vpi = vi[ref.intr_of_cam] if ref.intrinsics.shape[1] else np.zeros((len(vp), 0))
    out = {}
    for key, rows, cols_ in (("pose", vp, vp), ("intrinsics", vi, vi), ("pose_intrinsics", vp, vpi), ("points", vx, vx)):
        g = getattr(got, key)
        if g is not None:
            out[key] = block_error(g, getattr(ref, key), rows, cols_)
    return out


_CACHE = {}


def reference(name, arrays=None):
    """The long-double reference of case `name`, computed once per process -> namespace: ref (route B, long double), dev
    ({block type: deviation of the float64 evaluation}), bounds, pb, arrays, blocks, seconds.  `arrays`: host_arrays of the
    caller's own compiled problem (checked against the cached one's), default: compiled here on the CPU."""
    if name in _CACHE:
        if arrays is not None:
            for k in ("cam_q", "cam_t", "intr", "pts", "row_ptr", "obs_cam", "obs_uv"):
                assert np.array_equal(getattr(arrays, k), getattr(_CACHE[name].arrays, k)), f"{k}: another problem than the cached reference's"
        return _CACHE[name]
    t0 = time.time()
    case = SC.CASES[name]
    if arrays is None:
        arrays = SC.host_arrays(SC.compile_case(name, "cpu"), case)
    a = arrays
    pb = AG._Problem(a.cam_intr, a.row_ptr, a.obs_cam, a.obs_uv, a.model, a.refine_focal, a.refine_extra, a.loss, a.loss_scale,
                     a.cam_const, a.intr_const, a.pt_const, len(a.cam_t), len(a.intr), len(a.pts))
    blocks = pb.blocks(a.cam_q, a.cam_t, a.intr, a.pts)
    ref = schur_route(a, pb, blocks, LD)
    ref.intr_of_cam = a.cam_intr
    f64 = schur_route(a, pb, blocks, np.float64)
    dev = {k: v[0] for k, v in errors(f64, ref).items()}
    bounds = {k: max(SC.FLOOR_STEP, 100.0 * v) for k, v in dev.items()}
    out = SimpleNamespace(ref=ref, dev=dev, bounds=bounds, pb=pb, arrays=a, blocks=blocks, cost=blocks[0],
                          seconds=time.time() - t0)
    _CACHE[name] = out
    return out


# ------------------------------------------------------------------ seeded SPD matrices for vggc_spd_inverse
SPD_SIZES = (1, 14, 63, 64, 65, 127, 128, 129, 200, 770)


def spd_matrix(n, seed=0):
    """A = Q diag(w) Q^T + a banded part: Q from the QR factorisation of a seeded Gaussian matrix, eigenvalues w spread
    logarithmically over [1, 1e4] (condition 1e4: moderate), symmetrised exactly.  Row and column scales of up to 30 are put
    around it, as the columns of a reduced camera system differ (rotations, translations, focal lengths)."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    w = np.logspace(0, 4, n) if n > 1 else np.array([3.0])
    A = (Q * w) @ Q.T
    s = np.exp(rng.uniform(0, np.log(30.0), n))
    A = A * s[:, None] * s[None, :]
    return np.tril(A) + np.tril(A, -1).T


_SPD_CACHE = {}


def spd_reference(n):
    """(A float64, A^-1 long double, deviation of the float64 evaluation of cholesky_inverse from it, bound on that measure,
    bound on max |A X - I|: 100 x what the float64 evaluation leaves, at least FLOOR_STEP)."""
    if n not in _SPD_CACHE:
        A = spd_matrix(n)
        ref = cholesky_inverse(A.astype(LD))
        f64 = cholesky_inverse(A)
        d = np.diag(ref).astype(np.float64)
        dev = float((np.abs((f64 - ref).astype(np.float64)) / np.sqrt(np.outer(d, d))).max())
        res = float(np.abs(A @ f64 - np.eye(n)).max())           # (in float64, as the GPU test evaluates its own)
        _SPD_CACHE[n] = (A, ref, dev, max(SC.FLOOR_STEP, 100.0 * dev), max(SC.FLOOR_STEP, 100.0 * res))
    return _SPD_CACHE[n]
