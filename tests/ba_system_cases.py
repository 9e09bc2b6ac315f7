"""Shared by tests/test_ba_system_cases.py (CPU) and tests/test_gpu_ba_system.py: the case table of the bundle adjustment's
intermediates and a long-double reference for them -- reduce buffer 0 (per-camera U, g, cost), reduce buffer 1 (the reduced
camera system S | rhs), reduce buffer 2 (the points' gradient maximum) and the first Levenberg-Marquardt step.

The reference starts from a compiled problem's own arrays (`host_arrays`), so the camera order (`cam_perm`) and the point
numbering need no handling.  The Jacobian blocks and corrected residuals are oracle/ba_autograd's (`_Problem.blocks`:
torch.func.jacrev, sqrt(rho') correction); everything behind them is dense algebra in numpy, once in `numpy.longdouble` (the
reference) and once in float64 (`Reference.dev`: how far plain double arithmetic lands from it -- the GPU tests' bounds):

  Jacobi scale 1 / (1 + sqrt(colsq));  damping clip(colsq s^2, min_lm_diagonal, max_lm_diagonal) / radius on camera,
  intrinsics AND point columns;  S = A_cc - sum_p W_p V_p^-1 W_p^T,  rhs = b_c - sum_p W_p V_p^-1 b_p  (3 x 3 inverse by
  adjugate: numpy.linalg has no long double);  constant and unobserved columns carry zero Jacobians, so their rows of S hold
  the damping of a zero column on the diagonal and nothing else.  Then S y = rhs by a Cholesky factorisation written with
  numpy row operations (unit diagonal on the inactive columns), the points' back-substitution, x (+) (-y o scale) with
  ba_autograd's quaternion plus, the candidate's cost, the model cost change -J d . (r + J d / 2), |step| and |x|.

Reference against the C oracle (`oracle_first_iteration`: bao_debug_dump_system + iterations[1] of a one-iteration solve),
worst case over CASES, measured on x86-64 (80-bit long double) -- tests/test_ba_system_cases.py prints them:
  S (element error / sqrt(S_ii S_jj), active rows and columns)   6.35e-13  (case l_env; l 4.4e-13, h 1.7e-13, b 1.1e-13)
  rhs (error / max |rhs|, active rows)                            2.16e-14  (case l_env)
  cost_change, step_norm, relative_decrease (relative)            7.00e-12  (case l_env: step_norm; h 2.9e-12, g 2.0e-12)
The bounds are ten times these.  The worst cases are the ones whose reduced system is the worst conditioned (shared
intrinsics seen through short tracks); the float64 evaluation of the reference's own formulas is as far from the long-double
one there (S: l_env 1.4e-12) -- the oracle's double arithmetic, not a difference between the two derivations."""
import ctypes
import hashlib
import time
from types import SimpleNamespace

import numpy as np
import torch

import oracle.ba as OB
from oracle import ba_autograd as AG
from tests.test_gpu_ba_glue import window_scene
from vggsfm_amd import ba as BA
from vggsfm_amd.ba_options import LOSS_ID, BundleAdjustmentOptions
from vggsfm_amd.scene import make_scene, perturb_for_ba

LD = np.longdouble

ORACLE_SYSTEM_MEASURED = 6.35e-13
ORACLE_SYSTEM_BOUND = 10 * ORACLE_SYSTEM_MEASURED
ORACLE_RHS_MEASURED = 2.16e-14
ORACLE_RHS_BOUND = 10 * ORACLE_RHS_MEASURED
ORACLE_STEP_MEASURED = 7.00e-12
ORACLE_STEP_BOUND = 10 * ORACLE_STEP_MEASURED

# floors of the GPU tests' bounds (bound = max(floor, 100 x the float64 evaluation's deviation from the long-double one))
FLOOR_SUM, FLOOR_STEP = 1e-13, 1e-11


# ------------------------------------------------------------------ the cases
def _case(S, N, cam, shared, seed, scene="window", lo=3, hi=12, masked_frames=None, outlier_frac=0.05, full=False,
          refine_focal=True, refine_extra=True, loss="TRIVIAL", loss_scale=1.0, const_points=0, const_poses=None,
          filter_negative_depth=True, edge=""):
    return SimpleNamespace(**locals())


CASES = {
    "a": _case(2, 42, "SIMPLE_PINHOLE", False, 3, scene="plain", edge="two frames, n = 14"),
    "b": _case(16, 150, "SIMPLE_RADIAL", True, 4, lo=2, hi=6, edge="one full group, diagonal tile only, track length 2"),
    "c": _case(17, 150, "SIMPLE_RADIAL", True, 5, lo=2, hi=8, edge="second group of one camera, small off-diagonal tile"),
    "d": _case(33, 400, "SIMPLE_RADIAL", False, 6, edge="8 x 8 blocks, full factors, three groups"),
    "e": _case(33, 400, "SIMPLE_PINHOLE", False, 7, edge="7 x 7 blocks"),
    "f": _case(40, 300, "SIMPLE_PINHOLE", True, 8, lo=4, hi=30, edge="kd = 1, every tile populated"),
    "g": _case(48, 400, "SIMPLE_RADIAL", True, 9, lo=3, hi=36, masked_frames=(16, 32), edge="a group without observations"),
    "h": _case(20, 302, "SIMPLE_RADIAL", True, 10, outlier_frac=0.2, loss="CAUCHY", loss_scale=2.0, edge="loss-corrected blocks"),
    "i_focal": _case(24, 300, "SIMPLE_RADIAL", False, 11, refine_extra=False, edge="focal only: 7 x 7 blocks of a radial camera"),
    "i_extra": _case(24, 300, "SIMPLE_RADIAL", False, 11, refine_focal=False, edge="extra only: only_k"),
    "i_none": _case(24, 300, "SIMPLE_RADIAL", True, 11, refine_focal=False, refine_extra=False, edge="no intrinsics refined"),
    "j": _case(17, 302, "SIMPLE_RADIAL", True, 12, refine_focal=False, refine_extra=False, const_points=150,
               const_poses=(0, 1, 2, 3, 4), filter_negative_depth=False, edge="window BA: constant points and poses"),
    "k": _case(80, 122, "SIMPLE_RADIAL", True, 13, scene="plain", full=True, edge="32 lanes per point, long tracks, five groups"),
    "l": _case(80, 400, "SIMPLE_RADIAL", True, 14, lo=3, hi=10, edge="reordered cameras, two leading blocks"),
    "l_env": _case(128, 500, "SIMPLE_RADIAL", True, 15, lo=3, hi=10, edge="reordered cameras, row envelope"),
}
VARIANT_CASES = ("d", "f", "g")


def options_of(case, max_num_iterations=4):
    opt = BundleAdjustmentOptions()
    so = opt.solver_options
    so.max_num_iterations = max_num_iterations
    so.function_tolerance = so.gradient_tolerance = so.parameter_tolerance = 0.0
    opt.refine_focal_length, opt.refine_extra_params = case.refine_focal, case.refine_extra
    opt.loss_function_type, opt.loss_function_scale = case.loss, case.loss_scale
    return opt


def compile_case(name, device="cpu"):
    """The case's DeviceProblem on `device`, built the way BA.bundle_adjustment builds it (camera order, points numbered by
    track length, the constant blocks of a BundleAdjustmentConfig)."""
    c = CASES[name]
    if c.scene == "plain":
        sc = make_scene(c.S, c.N, c.cam, shared_camera=c.shared, seed=c.seed, full_visibility=c.full, outlier_frac=c.outlier_frac)
        mask = sc.mask
    else:
        sc, mask = window_scene(c.S, c.N, c.cam, c.shared, c.seed, lo=c.lo, hi=c.hi, masked_frames=c.masked_frames,
                                outlier_frac=c.outlier_frac)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=c.seed)
    T = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(device)
    prob, valid_idx, _ = BA.compile_problem(T(pts0), T(ext0), T(K0), T(sc.tracks), T(mask), T(extra0), c.shared, c.cam,
                                            filter_negative_depth=c.filter_negative_depth,
                                            gauge="colmap" if c.const_poses is None else "config", camera_split=True,
                                            refine_focal_length=c.refine_focal, refine_extra_params=c.refine_extra,
                                            sort_points=True)
    if c.const_poses is not None:
        cf = torch.as_tensor(list(c.const_poses), dtype=torch.long, device=prob.cam_const.device)
        if prob.cam_perm is not None:
            inv = torch.empty_like(prob.cam_perm)
            inv[prob.cam_perm] = torch.arange(c.S, device=prob.cam_perm.device)
            cf = inv[cf]
        prob.cam_const[cf] = 1
    if c.const_points:
        # (as window_bundle_adjustment: the first `const_points` VALID tracks, in track order)
        valid = torch.from_numpy(mask).to(device).sum(0) >= 2
        constant = valid & ((torch.cumsum(valid.long(), 0) - 1) < c.const_points)
        prob.pt_const = constant[valid_idx].to(torch.uint8).contiguous()
    return prob


def host_arrays(prob, case):
    """The problem's arrays on the host, in the types oracle.ba.solve_csr takes."""
    h = lambda t, dt: None if t is None else np.ascontiguousarray(t.detach().cpu().numpy().astype(dt))
    C, NI = prob.cam_t.shape[0], prob.intr.shape[0]
    return SimpleNamespace(
        cam_q=h(prob.cam_q, np.float64), cam_t=h(prob.cam_t, np.float64), intr=h(prob.intr, np.float64),
        pts=h(prob.pts, np.float64), row_ptr=h(prob.row_ptr, np.int32), obs_cam=h(prob.obs_cam, np.int32),
        obs_uv=h(prob.obs_uv, np.float64), cam_const=h(prob.cam_const, np.uint8), intr_const=h(prob.intr_const, np.uint8),
        pt_const=h(prob.pt_const, np.uint8), cam_intr=np.zeros(C, np.int32) if NI == 1 else np.arange(C, dtype=np.int32),
        model=prob.camera_model, refine_focal=bool(case.refine_focal), refine_extra=bool(case.refine_extra),
        loss=LOSS_ID[case.loss], loss_scale=float(case.loss_scale))


def tile_entry_counts(prob):
    """{(gI, gJ): entries} of the problem's Schur tiles."""
    cd = prob.chunk_desc.cpu().numpy()
    return {(int(r[0]), int(r[1])): int(r[3] - r[2]) for r in cd}


def check_edges(name, prob, merged=True):
    """Does the compiled problem reach the edge its case is in the table for?  `merged`: the tile launch form expected (every
    case is below MERGED_TILE_MAX_OBS observations)."""
    c = CASES[name]
    S = c.S
    tiles = tile_entry_counts(prob)
    G = -(-S // BA.GROUP)
    td = prob.tile_desc.cpu().numpy()
    assert sorted(tiles) == sorted((int(r[0]), int(r[1])) for r in td)
    counts = np.diff(prob.row_ptr.cpu().numpy())
    O, P = prob.num_obs, prob.pts.shape[0]
    kd = int(c.refine_focal) + int(c.refine_extra and c.cam == "SIMPLE_RADIAL")
    n = 6 * S + kd * (1 if c.shared else S)
    assert bool(prob.merged_tile_launch) == merged
    assert (prob.cam_perm is not None) == name.startswith("l")
    # some tile's entry count is no multiple of 4 (a quad padded with the zero segment), another's no multiple of 32 (a partial sub-chunk)
    odd4 = [t for t, k in tiles.items() if k % 4]
    odd32 = [t for t, k in tiles.items() if k % 32]
    assert odd4 and odd32 and (len(tiles) == 1 or len(set(odd4) | set(odd32)) >= 2), tiles
    auto_lanes = 16 if O / P <= 72.0 else 32             # (lanes_per_point / long_tracks in csrc/ba_types.hpp)
    auto_long = O > 1.5 * auto_lanes * P
    if name != "k":
        assert auto_lanes == 16 and not auto_long
    if name == "a":
        assert n == 14 and list(tiles) == [(0, 0)] and (counts == 2).all()
    elif name == "b":
        assert list(tiles) == [(0, 0)] and counts.min() == 2 and S == BA.GROUP
    elif name == "c":
        assert sorted(tiles) == [(0, 0), (0, 1), (1, 1)] and 0 < tiles[(0, 1)] <= 32 and tiles[(1, 1)] == tiles[(0, 1)]
    elif name in ("d", "e"):
        assert G == 3 and not c.shared and 6 + kd == (8 if name == "d" else 7)
        assert sorted(tiles) == [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2)]        # (tracks of <= 12 frames do not span three groups)
    elif name == "f":
        assert kd == 1 and c.shared and sorted(tiles) == [(i, j) for i in range(G) for j in range(i, G)] and G == 3
    elif name == "g":
        assert G == 3 and sorted(tiles) == [(0, 0), (0, 2), (2, 2)]
        cp = prob.col_ptr.cpu().numpy()
        assert (np.diff(cp)[16:32] == 0).all() and (np.diff(cp)[:16] > 0).all() and (np.diff(cp)[32:] > 0).all()
    elif name == "h":
        assert c.loss == "CAUCHY" and c.loss_scale == 2.0
    elif name == "i_focal":
        assert kd == 1 and not c.shared and c.refine_focal
    elif name == "i_extra":
        assert kd == 1 and not c.shared and not c.refine_focal
    elif name == "i_none":
        assert kd == 0 and c.shared and n == 6 * S
    elif name == "j":
        assert int(prob.pt_const.sum()) == c.const_points and prob.cam_const.cpu().tolist() == [1] * 5 + [0] * 12
        assert 0 < c.const_points < P
    elif name == "k":
        assert auto_lanes == 32 and auto_long and G == 5 and (counts == S).all()
    elif name.startswith("l"):
        perm = prob.cam_perm.cpu().numpy()
        assert sorted(perm.tolist()) == list(range(S)) and (perm != np.arange(S)).any()
        if name == "l":
            assert prob.chol_first_blk is None and tuple(prob.chol_split) != (0, 0)
            # (the smallest: two leading blocks need five full camera groups -- find_camera_split)
        else:
            assert prob.chol_first_blk is not None and int(prob.chol_first_blk.max()) > 0
        assert perm[0] == 0 and perm[1] == 1                                    # (the gauge frames stay in front)


# ------------------------------------------------------------------ the reference
def _rotmat(q):
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one = np.ones_like(x)
    return np.stack([one - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), one - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), one - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def observation_costs(a, obs_pt, q, t, intr, X, T):
    """rho(|r|^2) of every observation in the number type T (its own few lines: no torch, no oracle)."""
    q, t, intr, X, uv = (np.asarray(v).astype(T) for v in (q, t, intr, X, a.obs_uv))
    cam = a.obs_cam.astype(np.int64)
    Y = np.einsum("oij,oj->oi", _rotmat(q)[cam], X[obs_pt]) + t[cam]
    u, v = Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2]
    it = intr[a.cam_intr[cam]]
    d = 1 + it[:, 3] * (u * u + v * v) if a.model == 1 else np.ones_like(u)
    ru, rv = it[:, 0] * (d * u) + it[:, 1] - uv[:, 0], it[:, 0] * (d * v) + it[:, 2] - uv[:, 1]
    s = ru * ru + rv * rv
    if a.loss == 0:
        return s
    if a.loss == 1:
        b = T(a.loss_scale) * T(a.loss_scale)
        return b * np.log1p(s / b)
    raise NotImplementedError("the case table uses the trivial and the Cauchy loss")


def _inv3(V):
    """(P,3,3) symmetric -> inverses, by adjugate."""
    a, b, c, d, e, f = V[:, 0, 0], V[:, 0, 1], V[:, 0, 2], V[:, 1, 1], V[:, 1, 2], V[:, 2, 2]
    A, B, C = d * f - e * e, c * e - b * f, b * e - c * d
    D, E, F = a * f - c * c, b * c - a * e, a * d - b * b
    det = a * A + b * B + c * C
    return np.stack([A, B, C, B, D, E, C, E, F], 1).reshape(-1, 3, 3) / det[:, None, None]


def cholesky_solve(A, b):
    """A (lower triangle read) y = b in A's number type: right-looking Cholesky by row operations, two substitutions."""
    n = len(b)
    L = np.tril(A).copy()
    for j in range(n):
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
        if j + 1 < n:
            v = L[j + 1:, j]
            L[j + 1:, j + 1:] -= np.tril(np.outer(v, v))
    y = b.copy()
    for j in range(n):
        y[j] /= L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):
        y[j] /= L[j, j]
        y[:j] -= L[j, :j] * y[j]
    return y


def _evaluate(a, pb, blocks, so, T):
    """Buffers 0..2 and the first LM step from the per-observation blocks, all arithmetic in the number type T."""
    _, r, F, E, cols = blocks
    r, F, E = r.astype(T), F.astype(T), E.astype(T)
    C, P, nr, BD = pb.C, pb.P, pb.n_red, F.shape[2]
    cam, pt = pb.obs_cam, pb.obs_pt
    x = (a.cam_q, a.cam_t, a.intr, a.pts)
    out = SimpleNamespace()
    # reduce buffer 0: unscaled per-camera blocks
    out.U, out.g, out.cost = np.zeros((C, BD, BD), T), np.zeros((C, BD), T), np.zeros(C, T)
    np.add.at(out.U, cam, np.einsum("oki,okj->oij", F, F))
    np.add.at(out.g, cam, np.einsum("oki,ok->oi", F, r))
    np.add.at(out.cost, cam, observation_costs(a, pt, *x, T))
    # Jacobi scales and LM damping
    colsq_c, colsq_p = np.zeros(nr, T), np.zeros((P, 3), T)
    np.add.at(colsq_c, cols, (F * F).sum(1))
    np.add.at(colsq_p, pt, (E * E).sum(1))
    one = T(1)
    sc = one / (one + np.sqrt(colsq_c)) if so.jacobi_scaling else np.ones(nr, T)
    sp = one / (one + np.sqrt(colsq_p)) if so.jacobi_scaling else np.ones((P, 3), T)
    radius = T(so.initial_trust_region_radius)
    clip = lambda v: np.clip(v, T(so.min_lm_diagonal), T(so.max_lm_diagonal)) / radius
    damp_c, damp_p = clip(colsq_c * sc * sc), clip(colsq_p * sp * sp)
    Fs, Es = F * sc[cols][:, None, :], E * sp[pt][:, None, :]
    # camera side of the normal equations
    S, rhs = np.zeros((nr, nr), T), np.zeros(nr, T)
    np.add.at(S, (cols[:, :, None], cols[:, None, :]), np.einsum("oki,okj->oij", Fs, Fs))
    S[np.arange(nr), np.arange(nr)] += damp_c
    np.add.at(rhs, cols, np.einsum("oki,ok->oi", Fs, r))
    # point blocks and their elimination
    V, bp, gp = np.zeros((P, 3, 3), T), np.zeros((P, 3), T), np.zeros((P, 3), T)
    np.add.at(V, pt, np.einsum("oki,okj->oij", Es, Es))
    V[:, np.arange(3), np.arange(3)] += damp_p
    np.add.at(bp, pt, np.einsum("oki,ok->oi", Es, r))
    np.add.at(gp, pt, np.einsum("oki,ok->oi", E, r))
    pt_active = pb.active[nr::3]
    out.gmax_pts = np.abs(gp[pt_active]).max() if pt_active.any() else T(0)
    Vi = _inv3(V)
    W = np.einsum("oki,okj->oij", Fs, Es)                        # (O, BD, 3): the observation's rows of W_p
    row_ptr = a.row_ptr.astype(np.int64)
    for p in np.nonzero(pt_active)[0]:
        o0, o1 = row_ptr[p], row_ptr[p + 1]
        u, inv = np.unique(cols[o0:o1].ravel(), return_inverse=True)
        Wp = np.zeros((len(u), 3), T)
        np.add.at(Wp, inv.ravel(), W[o0:o1].reshape(-1, 3))
        WV = Wp @ Vi[p]
        S[np.ix_(u, u)] -= WV @ Wp.T
        rhs[u] -= WV @ bp[p]
    out.S, out.rhs = S, rhs
    out.scale_c, out.scale_p = sc, sp
    # first LM step
    act = pb.active[:nr]
    A, b = S.copy(), rhs.copy()
    for j in np.nonzero(~act)[0]:
        A[j, :], A[:, j], A[j, j], b[j] = 0, 0, 1, 0
    yc = cholesky_solve(A, b)
    tp = np.zeros((P, 3), T)
    np.add.at(tp, pt, np.einsum("oij,oi->oj", W, yc[cols]))
    yp = np.einsum("pij,pj->pi", Vi, bp - tp) * pt_active[:, None]
    Jd = -(np.einsum("oki,oi->ok", Fs, yc[cols]) + np.einsum("oki,oi->ok", Es, yp[pt]))
    out.model_change = -(Jd * (r + Jd / 2)).sum()
    out.delta = np.concatenate([-yc * sc, (-yp * sp).ravel()])
    out.cand = pb.plus(*x, out.delta.astype(np.float64))
    out.cost_x = out.cost.sum() / 2
    out.cost_cand = observation_costs(a, pt, *out.cand, T).sum() / 2
    out.cost_change = out.cost_x - out.cost_cand
    out.relative_decrease = out.cost_change / out.model_change
    out.step_norm = np.sqrt(sum(((u.astype(T) - v.astype(T)) ** 2).sum() for u, v in zip(x, out.cand)))
    out.x_norm = pb.x_norm(*x)
    return out


def quat_log_delta(q_new, q_old):
    """log(q_new (x) q_old^-1) of (x,y,z,w) unit quaternions, (C,3): the tangent step of the quaternion plus."""
    ax, ay, az, aw = q_new.T
    bx, by, bz, bw = -q_old[:, 0], -q_old[:, 1], -q_old[:, 2], q_old[:, 3]
    v = np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                  aw * bz + ax * by - ay * bx + az * bw], 1)
    w = aw * bw - ax * bx - ay * by - az * bz
    n = np.linalg.norm(v, axis=1)
    return v * np.where(n > 0, np.arctan2(n, w) / np.where(n > 0, n, 1.0), 1.0)[:, None]


def normalised_error(A, B, d):
    """max |A - B| / sqrt(d_i d_j) over the rows and columns with d > 0 (d: the REFERENCE's diagonal), lower triangle."""
    k = np.nonzero(d > 0)[0]
    s = np.sqrt(d[k])
    e = np.abs(np.tril(np.asarray(A - B)[np.ix_(k, k)])) / np.outer(s, s)
    return float(e.max()) if e.size else 0.0


def relative_to_max(a, b):
    m = float(np.abs(b).max())
    return float(np.abs(np.asarray(a - b)).max()) / m if m > 0 else float(np.abs(np.asarray(a)).max())


def step_errors(pb, x0, cand, cand_ref):
    """Errors of a candidate state against the reference's, per block type, relative to the reference step's largest
    component of that type: rotation (through log(q_new q_old^-1)), translation, intrinsics, points."""
    out = {}
    pairs = dict(rotation=(quat_log_delta(cand[0], x0[0]), quat_log_delta(np.asarray(cand_ref[0], np.float64), x0[0])),
                 translation=(cand[1] - x0[1], cand_ref[1] - x0[1]), intrinsics=(cand[2] - x0[2], cand_ref[2] - x0[2]),
                 points=(cand[3] - x0[3], cand_ref[3] - x0[3]))
    for key, (d, dref) in pairs.items():
        m = float(np.abs(dref).max())
        out[key] = float(np.abs(d - dref).max()) / m if m > 0 else float(np.abs(d).max())
    return out


def deviations(ev, ref, pb, x0):
    """The measures the GPU tests use, of one evaluation `ev` against the reference `ref`."""
    f = lambda v: float(abs(v))
    d = dict(
        U=max(normalised_error(ev.U[c], ref.U[c], np.diag(ref.U[c]).astype(np.float64)) for c in range(pb.C)),
        g=relative_to_max(ev.g, ref.g), cost=relative_to_max(ev.cost, ref.cost),
        S=normalised_error(ev.S, ref.S, np.where(pb.active[:pb.n_red], np.diag(ref.S), 0).astype(np.float64)),
        rhs=relative_to_max(ev.rhs, ref.rhs), gmax_pts=f(ev.gmax_pts - ref.gmax_pts) / f(ref.gmax_pts),
        cost_x=f(ev.cost_x - ref.cost_x) / f(ref.cost_x), cost_cand=f(ev.cost_cand - ref.cost_cand) / f(ref.cost_cand),
        cost_change=f(ev.cost_change - ref.cost_change) / f(ref.cost_change),
        step_norm=f(ev.step_norm - ref.step_norm) / f(ref.step_norm),
        relative_decrease=f(ev.relative_decrease - ref.relative_decrease) / f(ref.relative_decrease))
    d.update(step_errors(pb, x0, ev.cand, ref.cand))
    return d


_CACHE = {}


def reference(name, arrays):
    """The long-double reference of case `name` for `arrays` (host_arrays of its compiled problem), computed once per process.
    -> namespace: ref (long-double evaluation), dev (the float64 evaluation's deviations from it), bounds, pb, seconds."""
    a = arrays
    key = hashlib.sha1(b"".join(np.ascontiguousarray(v).tobytes() for v in (a.cam_q, a.cam_t, a.intr, a.pts, a.row_ptr, a.obs_cam,
                                                                           a.obs_uv, a.cam_const))).hexdigest()
    if name in _CACHE:
        assert _CACHE[name].key == key, "the case compiled to other arrays than the cached reference's"
        return _CACHE[name]
    t0 = time.time()
    so = options_of(CASES[name]).solver_options
    pb = AG._Problem(a.cam_intr, a.row_ptr, a.obs_cam, a.obs_uv, a.model, a.refine_focal, a.refine_extra, a.loss, a.loss_scale,
                     a.cam_const, a.intr_const, a.pt_const, len(a.cam_t), len(a.intr), len(a.pts))
    x0 = (a.cam_q, a.cam_t, a.intr, a.pts)
    blocks = pb.blocks(*x0)
    ref = _evaluate(a, pb, blocks, so, LD)
    f64 = _evaluate(a, pb, blocks, so, np.float64)
    assert abs(float(ref.cost_x) - blocks[0]) <= 1e-13 * blocks[0]          # (the two statements of the projection agree)
    dev = deviations(f64, ref, pb, x0)
    # (the candidate's cost is a function of the step -- it moves by gradient . step error --, so it is bounded like the step)
    step = ("cost_cand", "cost_change", "step_norm", "relative_decrease", "rotation", "translation", "intrinsics", "points")
    bounds = {k: max(FLOOR_STEP if k in step else FLOOR_SUM, 100.0 * v) for k, v in dev.items()}
    bounds["cost"] = bounds["cost_x"] = 1e-13                  # sums of squares at the start point, no cancellation
    out = SimpleNamespace(key=key, ref=ref, dev=dev, bounds=bounds, pb=pb, x0=x0, so=so, seconds=time.time() - t0)
    _CACHE[name] = out
    return out


def oracle_first_iteration(arrays):
    """One iteration of the C oracle on the arrays: (lhs (n,n), rhs (n,), summary)."""
    a = arrays
    kd = int(a.refine_focal) + int(a.refine_extra and a.model == 1)
    n = 6 * len(a.cam_t) + kd * len(a.intr)
    lhs, rhs = np.zeros((n, n)), np.zeros(n)
    L = OB.lib()
    L.bao_debug_dump_system.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.bao_debug_dump_system.restype = None
    L.bao_debug_dump_system(lhs.ctypes.data, rhs.ctypes.data)
    summ = OB.solve_csr(a.cam_q.copy(), a.cam_t.copy(), a.intr.copy(), a.pts.copy(), a.cam_intr, a.row_ptr, a.obs_cam, a.obs_uv,
                        a.model, OB.ceres_options(1, 0.0, 0.0, 0.0), refine_focal=a.refine_focal, refine_extra=a.refine_extra,
                        loss=a.loss, loss_scale=a.loss_scale, cam_const=a.cam_const, intr_const=a.intr_const, pt_const=a.pt_const)
    return lhs, rhs, summ
