"""The P3P minimal solver against a solver that does not share its method (a helper module, not a test file).

  solve                       the reference (numpy.longdouble, six Newton steps) and the float64 yardstick (two steps): the
                              quartic in v = d3/d1 by polynomial arithmetic, all four roots from numpy.roots (companion
                              matrix) -- no Ferrari, no resolvent, nothing of oracle/p3p.py -- u = d2/d1 from the common
                              root of the two quadratics, the pose as the affine map that takes the world triangle and
                              its normal to the camera triangle and its normal (M_cam M_world^-1 with the inverse written
                              out by cofactors; the oracle and the kernel build two orthonormal frames instead)
  FAMILIES, family, table     seeded noise-free triplets, T per family, with the reference, the conditioning filter and the
                              yardstick's solutions
  REGRESSION                  hand-written triplets (literal numbers) the solver lost before its resolvent was bracketed
  compare                     the two-direction comparison of a solver's <= 4 poses per triplet with the reference
  mp_poses                    the same solver in mpmath at 40 digits, for a spot check of the long-double path
"""
import functools

import numpy as np

LD = np.longdouble
T_PER_FAMILY = 2000
SEED = 20240
IMAG_TOL = 1e-8              # a root of numpy.roots is real when |imag| < IMAG_TOL (1 + |root|)
# a reference solution is left out of the tolerance checks when its root is closer than SEP_TOL (1 + |v|) to another root
# of the quartic (complex ones included), when |Q(v)| < SMALL_Q (|q1| + |q0|) (u = -P/Q is then badly determined) or when
# |k4| < SMALL_LEAD sum |k_i| (one root of the quartic runs off to infinity)
SEP_TOL, SMALL_Q, SMALL_LEAD = 1e-3, 1e-3, 1e-6
CAP = 0.03                   # at most this share of a family's reference solutions is left out; table() asserts it
MARGIN = 10.0                # the bound of the solver under test: one decade above the yardstick's largest error

FAMILIES = ("generic", "equal_depths", "d1_eq_d2", "d1_eq_d3", "a23_eq_a12", "a13_eq_a12", "wide", "fronto_parallel",
            "depth_ratio_100", "scaled_1e3")

# The float64 yardstick (solve(..., float64, 2)) against the long-double reference over the kept solutions of table(),
# T_PER_FAMILY = 2000 triplets per family, SEED = 20240, measured on the CPU (x86-64, 80-bit long double):
# family -> (largest max|d[R|t]| / (1 + max|[R|t]|), largest |dv| / v).  DESIGN.md section 18 has the shares left out.
YARDSTICK = {
    "generic": (6.31e-10, 1.94e-10), "equal_depths": (1.10e-06, 1.91e-08), "d1_eq_d2": (1.27e-08, 4.37e-10),
    "d1_eq_d3": (1.07e-06, 2.08e-08), "a23_eq_a12": (1.77e-08, 2.65e-10), "a13_eq_a12": (4.88e-09, 2.69e-11),
    "wide": (1.22e-09, 3.86e-11), "fronto_parallel": (2.55e-07, 4.77e-09), "depth_ratio_100": (2.80e-11, 1.85e-11),
    "scaled_1e3": (3.65e-09, 1.26e-10),
}
# numpy.roots is LAPACK's eigensolver: another build of it moves the last bits of a start value and with them the worst
# case of 2000; the yardstick has to stay within this factor of what was recorded
YARDSTICK_SLACK = 3.0
# the generating pose against the reference solution nearest to it: the inputs are the exact scene rounded to float64
# (2^-53 relative), a kept solution amplifies that by at most ~1 / SEP_TOL^2, an ill-conditioned one by more
TRUE_POSE_BOUND = 1e-7
# every reference pose has to reproduce the directions of its three points to this, times the scale of the triplet
# (tests/test_p3p_cases.py), in long double (eps 1.1e-19)
REPROJECTION_BOUND = 1e-15
# the reference against the same solver in mpmath at 40 digits, kept solutions: long double carries 11 bits more than
# float64, so its error has to be a small share of the yardstick's largest (1 / 2048 at the same amplification)
MP_SHARE = 0.01


def bound(name):
    """pose bound of the solver under test on a family"""
    return MARGIN * YARDSTICK[name][0]


# --- scenes ----------------------------------------------------------------------------------------------------------------
def _rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def _unit(x):
    b = np.concatenate([x, np.ones(x.shape[:-1] + (1,))], -1)
    return b / np.linalg.norm(b, axis=-1, keepdims=True)


def _third_distance(b, d, apex):
    """d3 along bearing 3 with |Y_apex - d3 b3| = |Y1 - Y2| (the larger root); NaN where there is none"""
    Y = d[:, :2, None] * b[:, :2]
    a12 = ((Y[:, 0] - Y[:, 1]) ** 2).sum(1)
    proj = (b[:, 2] * Y[:, apex]).sum(1)
    with np.errstate(invalid="ignore"):
        return proj + np.sqrt(proj * proj - (Y[:, apex] ** 2).sum(1) + a12)


def family(name, T=T_PER_FAMILY, seed=SEED):
    """dict(x (T,3,2) normalised image points, X (T,3,3) world points, pose (T,3,4) the generating [R|t]).  d is the
    distance of a point from the camera centre (the solver's d_i), not its z."""
    rng = np.random.default_rng(seed + FAMILIES.index(name))
    n = 4 * T                                                    # the two constrained families reject some draws
    x = rng.uniform(-1.0, 1.0, (n, 3, 2))
    d = rng.uniform(2.0, 6.0, (n, 3))
    ok = np.ones(n, bool)
    scale = 1.0
    if name == "equal_depths":
        d[:, 1] = d[:, 2] = d[:, 0]
    elif name == "d1_eq_d2":
        d[:, 1] = d[:, 0]
    elif name == "d1_eq_d3":
        d[:, 2] = d[:, 0]
    elif name in ("a23_eq_a12", "a13_eq_a12"):                   # A2 = 0: no u^2 in the second quadratic / c10 = 0
        d[:, 2] = _third_distance(_unit(x), d, 1 if name == "a23_eq_a12" else 0)
        with np.errstate(invalid="ignore"):
            ok = (d[:, 2] > 1.0) & (d[:, 2] < 8.0)
    elif name == "wide":
        x = rng.uniform(-3.0, 3.0, (n, 3, 2))
    elif name == "fronto_parallel":                              # the plane z = 4 of the camera frame
        d = 4.0 * np.linalg.norm(np.concatenate([x, np.ones((n, 3, 1))], -1), axis=-1)
    elif name == "depth_ratio_100":
        d[:, 0], d[:, 1] = 0.5, 50.0
        d = np.take_along_axis(d, np.argsort(rng.random((n, 3)), axis=1), 1)
    elif name == "scaled_1e3":
        scale = 1e3
    R = _rotations(rng, n)
    t = 3.0 * rng.normal(size=(n, 3))
    keep = np.nonzero(ok)[0][:T]
    assert len(keep) == T, name
    x, d, R, t = x[keep], d[keep], R[keep], t[keep] * scale
    Y = (d * scale)[..., None] * _unit(x)
    X = np.einsum("tji,tnj->tni", R, Y - t[:, None])
    return dict(x=x, X=X, pose=np.concatenate([R, t[..., None]], -1))


# --- the solver ------------------------------------------------------------------------------------------------------------
def _pmul(a, b):
    """product of two polynomials, coefficients along the last axis, lowest degree first"""
    out = np.zeros(a.shape[:-1] + (a.shape[-1] + b.shape[-1] - 1,), a.dtype)
    for i in range(a.shape[-1]):
        for j in range(b.shape[-1]):
            out[..., i + j] += a[..., i] * b[..., j]
    return out


def _pval(c, v):
    """c (T,n) at v (T,k)"""
    out = np.zeros_like(v)
    for i in range(c.shape[-1] - 1, -1, -1):
        out = out * v + c[:, i:i + 1]
    return out


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _triangle_matrix(P1, P2, P3):
    """columns P2 - P1, P3 - P1 and their cross product"""
    e, f = P2 - P1, P3 - P1
    return np.stack([e, f, _cross(e, f)], -1)


def _inverse3(M):
    """inverse of 3x3 matrices by cofactors (numpy.linalg has no long double)"""
    a, b, c = M[..., 0], M[..., 1], M[..., 2]
    bc = _cross(b, c)
    det = (a * bc).sum(-1)
    return np.stack([bc, _cross(c, a), _cross(a, b)], -2) / det[..., None, None]


def quartic(x, X, dt):
    """The two distance-ratio equations in u = d2/d1, v = d3/d1 (law of cosines in the three faces of the tetrahedron
    camera centre + triangle, divided by d1^2 and by each other):
        a1 u^2 + b1 u + C1(v) = 0,   a2 u^2 + B2(v) u + C2(v) = 0
    a1 eq2 - a2 eq1 is linear in u: P(v) + Q(v) u = 0, and the resultant K = P^2 - Q (b1 C2 - B2 C1) is a quartic in v.
    Returns dict(K (T,5), P (T,3), Q (T,2), lowest degree first, c12, a12, b (T,3,3) bearings)."""
    x, X = x.astype(dt), X.astype(dt)
    b = np.concatenate([x, np.ones(x.shape[:-1] + (1,), dt)], -1)
    b = b / np.sqrt((b * b).sum(-1, keepdims=True))
    sq = lambda i, j: ((X[:, i] - X[:, j]) ** 2).sum(-1)
    cs = lambda i, j: (b[:, i] * b[:, j]).sum(-1)
    a12, a13, a23 = sq(0, 1), sq(0, 2), sq(1, 2)
    c12, c13, c23 = cs(0, 1), cs(0, 2), cs(1, 2)
    A13, A23 = a13 / a12, a23 / a12
    one, zero = np.ones_like(a12), np.zeros_like(a12)
    const = lambda v: v[:, None]
    a1, b1, C1 = const(A13), const(-2 * A13 * c12), np.stack([A13 - 1, 2 * c13, -one], -1)
    a2, B2, C2 = const(A23 - 1), np.stack([-2 * A23 * c12, 2 * c23], -1), np.stack([A23, zero, -one], -1)
    P = a1 * C2 - a2 * C1
    Q = a1 * B2 - a2 * np.concatenate([b1, const(zero)], -1)
    K = _pmul(P, P) - _pmul(Q, np.concatenate([b1 * C2, const(zero)], -1) - _pmul(B2, C1))
    return dict(K=K, P=P, Q=Q, c12=c12, a12=a12, b=b, X=X)


def solve(x, X, dt=LD, newton=6):
    """x (T,3,2), X (T,3,3) -> dict(pose (T,4,3,4), valid (T,4), v, u (T,4), keep (T,4) = valid and well conditioned,
    roots (T,4) complex, and the polynomials of quartic())"""
    q = quartic(x, X, dt)
    K, P, Q = q["K"], q["P"], q["Q"]
    T = len(x)
    roots = np.full((T, 4), np.nan + 0j)
    K64 = K.astype(np.float64)
    for t in range(T):
        if np.isfinite(K64[t]).all():
            r = np.roots(K64[t, ::-1])
            roots[t, :len(r)] = r
    with np.errstate(all="ignore"):
        real = np.abs(roots.imag) < IMAG_TOL * (1.0 + np.abs(roots))
        v = np.where(real, roots.real, 1.0).astype(dt)
        dK = K[:, 1:] * np.arange(1, 5).astype(dt)
        for _ in range(newton):
            v = v - _pval(K, v) / _pval(dK, v)
        Qv = _pval(Q, v)
        u = -_pval(P, v) / Qv
        valid = real & (v > 0) & (u > 0) & np.isfinite(u.astype(np.float64))
        vr = v.astype(np.float64)                                    # every real root, valid or not
        u, v = np.where(valid, u, 1.0), np.where(valid, v, 1.0)
        d1 = np.sqrt(q["a12"][:, None] / (1 + u * u - 2 * u * q["c12"][:, None]))
        b = q["b"][:, None]                                          # (T,1,3,3)
        Y = np.stack([d1, u * d1, v * d1], -1)[..., None] * b        # (T,4,3,3)
        Mc = _triangle_matrix(Y[:, :, 0], Y[:, :, 1], Y[:, :, 2])
        Mw = _inverse3(_triangle_matrix(q["X"][:, 0], q["X"][:, 1], q["X"][:, 2]))[:, None]
        R = (Mc[..., :, :, None] * Mw[..., None, :, :]).sum(-2)
        t = Y[:, :, 0] - (R * q["X"][:, None, None, 0]).sum(-1)
        pose = np.concatenate([R, t[..., None]], -1)
        valid &= np.isfinite(pose.astype(np.float64)).all((-1, -2))
        pose = np.where(valid[..., None, None], pose, 0.0)
        # conditioning
        full = np.where(real, vr + 0j, roots)
        dist = np.abs(full[:, :, None] - full[:, None, :])
        dist[:, np.arange(4), np.arange(4)] = np.inf
        dist = np.where(np.isnan(dist), np.inf, dist)
        near = dist.min(2) < SEP_TOL * (1.0 + np.abs(v.astype(np.float64)))
        small_q = np.abs(Qv) < SMALL_Q * np.abs(Q).sum(-1, keepdims=True)
        small_lead = (np.abs(K[:, 4]) < SMALL_LEAD * np.abs(K).sum(-1))[:, None]
        keep = valid & ~(near | small_q | small_lead)
    return dict(q, pose=pose, valid=valid, keep=keep, v=v, u=u, roots=roots)


# --- comparison ------------------------------------------------------------------------------------------------------------
def pose_errors(ref_pose, ref_valid, pose, valid):
    """E (T,4,4): max|ref_i - pose_s| / (1 + max|ref_i|), inf where either is invalid"""
    ref = ref_pose.astype(np.float64)
    with np.errstate(all="ignore"):
        E = np.abs(ref[:, :, None] - pose.astype(np.float64)[:, None]).max((-1, -2)) / (1.0 + np.abs(ref).max((-1, -2)))[:, :, None]
    return np.where(ref_valid[:, :, None] & valid[:, None, :], E, np.inf)


def compare(ref, pose, valid, tol):
    """ref = a solve() result.  Returns (missed, spurious): lists of (triplet, solution index, error), worst first.
    missed: kept reference solutions without a valid pose within tol.  spurious: valid poses further than tol from every
    reference solution, on the triplets all of whose reference solutions are kept."""
    E = pose_errors(ref["pose"], ref["valid"], pose, valid)
    e1 = E.min(2)
    missed = [(int(t), int(i), float(e1[t, i])) for t, i in zip(*np.nonzero(ref["keep"] & ~(e1 <= tol)))]
    e2 = E.min(1)
    clean = (ref["keep"] == ref["valid"]).all(1)
    spurious = [(int(t), int(s), float(e2[t, s])) for t, s in zip(*np.nonzero(valid & clean[:, None] & ~(e2 <= tol)))]
    key = lambda m: -m[2]
    return sorted(missed, key=key), sorted(spurious, key=key)


def describe(name, what, found, total):
    worst = ", ".join(f"triplet {t} solution {i}: {e:.2e}" for t, i, e in found[:5])
    return f"{name}: {len(found)} of {total} {what} (bound {bound(name):.2e}); worst: {worst}"


# --- the table -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table():
    """name -> dict(x, X, pose of family(), ref = solve() in long double, yard = solve() in float64 with two steps)"""
    out = {}
    for name in FAMILIES:
        f = family(name)
        f["ref"] = solve(f["x"], f["X"], LD, 6)
        f["yard"] = solve(f["x"], f["X"], np.float64, 2)
        share = left_out_share(f["ref"])
        assert share <= CAP, f"{name}: {share:.4f} of the reference solutions are left out, the cap is {CAP}"
        out[name] = f
    return out


def left_out_share(ref):
    return 1.0 - ref["keep"].sum() / max(int(ref["valid"].sum()), 1)


def yardstick_errors(f):
    """(largest pose error, largest |dv| / v) of the yardstick over the kept reference solutions"""
    ref, yard = f["ref"], f["yard"]
    E = pose_errors(ref["pose"], ref["valid"], yard["pose"], yard["valid"])
    s = E.argmin(2)
    dv = np.abs(np.take_along_axis(yard["v"].astype(LD), s, 1) - ref["v"]) / ref["v"]
    k = ref["keep"]
    return float(E.min(2)[k].max()), float(dv[k].max())


# --- regression triplets -----------------------------------------------------------------------------------------------------
# name -> (family it was drawn from, x (3,2), X (3,3), generating pose (3,4)); literal numbers
# complex_pair_right_*: the resolvent has one real root and a complex pair to its right (0.310 and 1.495 +- 0.254i;
#   0.00438 and 0.1393 +- 0.0300i): Newton from the Cauchy bound never reached the real root, all four roots came out invalid
# small_lead_*: |k4| = 5.1e-5 and 4.6e-5 of sum |k_i|: the depressed coefficients are ~1e6, ~1e12, ~1e18, the start value
#   ~1e19 and the root ~1e6; 80 Newton steps at a contraction of 2/3 did not arrive
REGRESSION = {
    "complex_pair_right_a": ("generic",
        [[0.6414524805881865, 0.21370232236251718], [-0.4782619175335763, -0.04236613752189178],
         [0.9103289815678248, 0.10573140929864655]],
        [[2.503584373810247, -0.6968473702805595, 0.1810347928846483], [2.74498754010582, 2.7417229076583003, -1.652979520119585],
         [0.8595870600469441, -1.6780395570892739, -0.7277006548884937]],
        [[-0.47845043353061056, -0.877856730718727, -0.021277758016263693, 1.7286570674427528],
         [-0.5668848989943491, 0.29027744501307406, 0.7709607747537148, 1.8613134676155523],
         [-0.6706166520051056, 0.38092855661988634, -0.6365270935356584, 3.834811980962874]]),
    "complex_pair_right_b": ("generic",
        [[-0.03293485603461188, -0.7603266857554418], [0.8743613999469952, -0.4442257805487533],
         [0.0011708783263622013, -0.4899295217516242]],
        [[-4.770564929575903, 3.024327576562452, 10.772094366840129], [-6.751582009511424, 5.574541206153089, 10.793011166725446],
         [-5.451802918973662, 3.351956308831059, 12.600802688182338]],
        [[-0.42258534003038783, 0.8658498843801512, -0.26781637013125276, -1.8264284085086717],
         [-0.7799734025073806, -0.4979287567811106, -0.37908896653882884, 0.09587748371226433],
         [-0.4615876100725204, 0.04869220563186988, 0.8857572733758625, -9.559270405367332]]),
    "small_lead_a": ("generic",
        [[0.700114253719128, 0.3409397744951579], [-0.37712652629893806, 0.916483759452263],
         [-0.15244516462576008, -0.9681703248515006]],
        [[3.168940147711264, -8.234408977207494, -5.808283045163124], [1.5090886791596123, -10.015615801140717, -2.760503854881086],
         [-1.1341443608826172, -6.227097742002504, -6.446952555064816]],
        [[0.7891369375011306, 0.17832851556710916, -0.587760014297475, -2.241495779420436],
         [0.5623323008534422, -0.5946899213070793, 0.5745661675670204, -2.2680460185982336],
         [-0.24707342489270376, -0.7839278270551511, -0.5695716677296883, -5.831428113065252]]),
    "small_lead_b": ("generic",
        [[-0.5614724712583725, 0.9827606833338685], [-0.7725195832394907, -0.013325696247417973],
         [0.5113268417419434, 0.47122453661911345]],
        [[-2.879391533434595, 7.31387675377288, -5.684455922489779], [-4.006122032420645, 10.172499651561221, -3.045760870352075],
         [-1.5994165403438072, 6.343445302358308, -1.2938877414092462]],
        [[0.7625573287375822, -0.4549615835165118, 0.4599089887279342, 5.920364956124306],
         [0.12650103653179617, -0.5923288710328445, -0.7957034600259927, 4.054153765952671],
         [0.6344318782540677, 0.6649484687290463, -0.3941316097319676, -1.3280920695822616]]),
}
# thin_triangle_gate: X1 and X2 0.013 apart, the third point 3 away: A13 = 5.3e4; the consistency gate compared the residuals
#   of the two quadratics with 1 + u^2 + v^2 instead of with their own terms and dropped both (correct) solutions
REGRESSION["thin_triangle_gate"] = ("d1_eq_d2",
    [[-0.8091798003114405, 0.049382060823169205], [-0.8119448528237647, 0.0562665754251932],
     [0.9256532335369059, -0.7513379705976144]],
    [[1.7759518909315424, 1.5411226766220985, 4.3139254271132215], [1.7841176341244367, 1.539888473592344, 4.30359036140152],
     [1.457169557086801, -0.7172533946821269, 6.344918586719714]],
    [[0.3010943356798572, -0.7454822778048036, 0.5946413831045291, -3.451934463743293],
     [0.8244480822466578, -0.10985191018819385, -0.5551737723522371, 1.191686004440812],
     [0.47919470020161314, 0.6574106260983062, 0.5815356463637626, -2.5181035624081924]])
# reversed_small_lead: |k4| = 7.7e-6 of sum |k_i|, roots 0.384, 0.406, 1.31 and 2.9e4: Ferrari on the quartic itself shifts by
#   b / 4 = 7216 and sees the first two, 0.02 apart, as a complex pair; it is solved in 1 / v now
REGRESSION["reversed_small_lead"] = ("generic",
    [[0.3630371471944469, -0.8184559760158345], [-0.7120475413945331, 0.16051032766027262],
     [-0.9880487262242077, -0.3064910769824396]],
    [[3.6092191743154896, -4.35213998974513, -1.2360249037074689], [5.173505419966427, -1.8505269307657881, 3.654840932125846],
     [3.6126615019348587, -3.290756261084958, 3.765144936859957]],
    [[0.23082883985736047, -0.008941546975356207, -0.9729532853265839, -0.9461986431239424],
     [0.372279403511233, 0.9246816865845756, 0.07982370710775843, 0.2353765905343397],
     [0.8989583374169383, -0.3806360824104727, 0.2167719547261182, -1.5248995653219304]])
# The yardstick on the regression triplets themselves, where it exceeds its family's largest error (measured as above)
REGRESSION_YARDSTICK = {"thin_triangle_gate": 2.07e-07}


def regression_bound(name):
    return MARGIN * max(YARDSTICK[REGRESSION[name][0]][0], REGRESSION_YARDSTICK.get(name, 0.0))


# The resolvent the issue names for the first cause, m^3 + p m^2 + c1 m + c0 with roots 0.00428 and 0.2076 +- 0.0144i,
# as a depressed quartic y^4 + p y^2 + q y + r (r = p^2/4 - c1, q = sqrt(-8 c0)); its real roots are simple
RESOLVENT_CASE = dict(p=-0.4195, c1=0.04509, c0=-1.854e-4)


@functools.lru_cache(maxsize=None)
def regression():
    """name -> dict(family, x (1,3,2), X (1,3,3), pose (1,3,4), ref, bound)"""
    out = {}
    for name, (fam, x, X, pose) in REGRESSION.items():
        x, X, pose = (np.array(a, np.float64)[None] for a in (x, X, pose))
        out[name] = dict(family=fam, x=x, X=X, pose=pose, ref=solve(x, X, LD, 6), bound=regression_bound(name))
    return out


# --- mpmath ------------------------------------------------------------------------------------------------------------------
def mp_poses(x, X, digits=40):
    """One triplet in mpmath: list of (v, pose 3x4 as nested lists of mpf) for the real roots v > 0 with u > 0.  The same
    equations, written out with scalars; the roots from mpmath.polyroots."""
    import mpmath as mp
    with mp.workdps(digits):
        f = lambda a: mp.mpf(float(a))
        b = []
        for i in range(3):
            w = [f(x[i][0]), f(x[i][1]), mp.mpf(1)]
            n = mp.sqrt(sum(c * c for c in w))
            b.append([c / n for c in w])
        Xw = [[f(c) for c in X[i]] for i in range(3)]
        sq = lambda i, j: sum((Xw[i][k] - Xw[j][k]) ** 2 for k in range(3))
        cs = lambda i, j: sum(b[i][k] * b[j][k] for k in range(3))
        a12, A13, A23 = sq(0, 1), sq(0, 2) / sq(0, 1), sq(1, 2) / sq(0, 1)
        c12, c13, c23 = cs(0, 1), cs(0, 2), cs(1, 2)
        a1, b1, a2 = A13, -2 * A13 * c12, A23 - 1
        C1 = lambda v: -v * v + 2 * c13 * v + A13 - 1
        B2 = lambda v: 2 * c23 * v - 2 * A23 * c12
        C2 = lambda v: A23 - v * v
        res = lambda v: (a1 * C2(v) - a2 * C1(v)) ** 2 - (a1 * B2(v) - a2 * b1) * (b1 * C2(v) - B2(v) * C1(v))
        # the quartic's coefficients by interpolation at five points (exact up to the working precision)
        pts = [mp.mpf(k) for k in (-2, -1, 0, 1, 2)]
        V = mp.matrix([[p ** (4 - j) for j in range(5)] for p in pts])
        coef = mp.lu_solve(V, mp.matrix([res(p) for p in pts]))
        out = []
        for r in mp.polyroots(list(coef), maxsteps=200, extraprec=200):
            if abs(mp.im(r)) > mp.mpf(10) ** (-digits // 2) * (1 + abs(r)) or mp.re(r) <= 0:
                continue
            v = mp.re(r)
            u = -(a1 * C2(v) - a2 * C1(v)) / (a1 * B2(v) - a2 * b1)
            if u <= 0:
                continue
            d1 = mp.sqrt(a12 / (1 + u * u - 2 * u * c12))
            Y = [[d * c for c in b[i]] for i, d in enumerate((d1, u * d1, v * d1))]
            cr = lambda p, q: [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]
            tri = lambda P: mp.matrix([[P[1][k] - P[0][k], P[2][k] - P[0][k],
                                        cr([P[1][j] - P[0][j] for j in range(3)], [P[2][j] - P[0][j] for j in range(3)])[k]]
                                       for k in range(3)])
            R = tri(Y) * mp.inverse(tri(Xw))
            t = mp.matrix(Y[0]) - R * mp.matrix(Xw[0])
            out.append((v, [[R[i, 0], R[i, 1], R[i, 2], t[i]] for i in range(3)]))
        return out
