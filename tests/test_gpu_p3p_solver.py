"""GPU: the minimal solver of vgg_p3p_ransac (p3p_hypotheses_kernel) against the long-double reference of tests/p3p_cases.py
-- every kept reference solution found, no valid solution spurious, within one decade of the float64 yardstick -- and bit for
bit against oracle/p3p.py, read from the caller's workspace (layout: include/vggsfm_amd.h); and the three kernels at the
shapes where their indexing can go wrong, bit for bit against oracle.p3p.absolute_pose_ransac."""
import numpy as np
import pytest
import torch

from oracle import p3p as P
from tests import p3p_cases as C
from vggsfm_amd import _lib

pytestmark = pytest.mark.gpu


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run(x, X, mask, samples, thr_sq, group=1):
    """vgg_p3p_ransac through the C-ABI with a workspace of the test's own.  x (F,N,2), X (N,3), mask (F,N) bool or None,
    samples (F/group,H,3), thr_sq (F,).  Returns dict(pose, num, rsum, best, inl, hyp (F,H,4,3,4), valid (F,H,4) bool)."""
    L = _lib.lib()
    F, N, H = x.shape[0], x.shape[1], samples.shape[1]
    dx, dX, dthr = D(x.astype(np.float64)), D(X.astype(np.float64)), D(np.asarray(thr_sq, np.float64))
    dm = None if mask is None else D(mask.astype(np.uint8))
    ds = D(samples.astype(np.int32))
    pose = torch.full((F, 3, 4), 7.0, dtype=torch.float64, device="cuda")
    num = torch.full((F,), 7, dtype=torch.int32, device="cuda")
    rsum = torch.full((F,), 7.0, dtype=torch.float64, device="cuda")
    best = torch.full((F,), 7, dtype=torch.int32, device="cuda")
    inl = torch.full((F, N), 7, dtype=torch.uint8, device="cuda")
    nbytes = L.vgg_p3p_ransac_workspace_bytes(F, H)
    fh = F * H
    assert nbytes >= fh * (48 * 8 + 4 * 8 + 4 * 4 + 4)
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    _lib.check(L.vgg_p3p_ransac(dx, dX, dm, ds, F, group, N, H, dthr, pose, num, rsum, best, inl, ws, _lib.stream_ptr()),
               "vgg_p3p_ransac")
    torch.cuda.current_stream().synchronize()
    w = ws.cpu().numpy()
    hyp = w[:fh * 48 * 8].view(np.float64).reshape(F, H, 4, 3, 4).copy()
    off = fh * (48 * 8 + 4 * 8 + 4 * 4)
    valid = w[off:off + fh * 4].reshape(F, H, 4)
    assert ((valid == 0) | (valid == 1)).all()
    return dict(pose=pose.cpu().numpy(), num=num.cpu().numpy(), rsum=rsum.cpu().numpy(), best=best.cpu().numpy(),
                inl=inl.cpu().numpy(), hyp=hyp, valid=valid.astype(bool))


def solve_on_device(x, X):
    """x (T,3,2), X (T,3,3) -> (poses (T,4,3,4), valid (T,4)): N = 3 T points, one frame, sample h = (3h, 3h+1, 3h+2)"""
    T = len(x)
    r = run(x.reshape(1, 3 * T, 2), X.reshape(3 * T, 3), None, np.arange(3 * T, dtype=np.int32).reshape(1, T, 3), [1e-6])
    return r["hyp"][0], r["valid"][0]


@pytest.fixture(scope="module")
def table():
    return C.table()


@pytest.mark.parametrize("name", C.FAMILIES)
def test_device_solver_against_reference_and_oracle(table, name):
    f = table[name]
    poses, ok = solve_on_device(f["x"], f["X"])
    missed, spurious = C.compare(f["ref"], poses, ok, C.bound(name))
    lines = []
    if missed:
        lines.append(C.describe(name, "kept reference solutions have no valid solution", missed, int(f["ref"]["keep"].sum())))
    if spurious:
        lines.append(C.describe(name, "valid solutions are no reference solution", spurious, int(ok.sum())))
    E = C.pose_errors(f["ref"]["pose"], f["ref"]["valid"], poses, ok).min(2)[f["ref"]["keep"]]
    print(f"{name}: {int(ok.sum())} valid device solutions, worst kept {E.max():.2e} (bound {C.bound(name):.2e})")
    assert not lines, "\n" + "\n".join(lines)
    po, oo = P.p3p_solve(f["x"], f["X"])
    np.testing.assert_array_equal(ok, oo)
    np.testing.assert_array_equal(poses.view(np.uint64), po.view(np.uint64))


@pytest.mark.parametrize("name", sorted(C.REGRESSION))
def test_device_recovers_regression_triplet(name):
    r = C.regression()[name]
    ref = r["ref"]
    poses, ok = solve_on_device(r["x"], r["X"])
    missed, spurious = C.compare(ref, poses, ok, r["bound"])
    assert not missed and not spurious, (missed, spurious)
    i = int(np.argmin(C.pose_errors(ref["pose"], ref["valid"], r["pose"][:, None], np.ones((1, 1), bool))[0, :, 0]))
    assert ref["keep"][0, i] and C.pose_errors(ref["pose"], ref["valid"], poses, ok)[0, i].min() <= r["bound"]
    po, oo = P.p3p_solve(r["x"], r["X"])
    np.testing.assert_array_equal(ok, oo)
    np.testing.assert_array_equal(poses.view(np.uint64), po.view(np.uint64))


# --- the three kernels at the edges of their indexing -------------------------------------------------------------------------
INT_POSE = np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 3.0]])     # small integers


def scene(N, F, seed, outliers=0.25, noise=2e-4):
    """F cameras on N shared points: X (N,3), x (F,N,2) with noise and gross outliers (never among the first three points)"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (N, 3))
    x = np.empty((F, N, 2))
    for f in range(F):
        Pm = np.concatenate([C._rotations(rng, 1)[0], [[rng.uniform(-0.3, 0.3)], [rng.uniform(-0.3, 0.3)], [4.0]]], 1)
        Y = X @ Pm[:, :3].T + Pm[:, 3]
        x[f] = Y[:, :2] / Y[:, 2:] + noise * rng.normal(size=(N, 2))
        bad = rng.random(N) < outliers
        bad[:3] = False
        x[f, bad] += rng.uniform(-0.5, 0.5, (int(bad.sum()), 2))
    return X, x


def draw(rng, sets, H, N):
    return np.stack([np.stack([rng.choice(N, 3, replace=False) for _ in range(H)]) for _ in range(sets)]).astype(np.int32)


def check_against_oracle(r, x, X, mask, samples, thr_sq, group=1):
    F, N = x.shape[:2]
    for f in range(F):
        m = np.ones(N, bool) if mask is None else mask[f]
        o = P.absolute_pose_ransac(x[f], X, m, samples[f // group], thr_sq[f])
        assert int(r["num"][f]) == o["num_inliers"] and int(r["best"][f]) == o["best"], (f, r["num"][f], o["num_inliers"], r["best"][f], o["best"])
        np.testing.assert_array_equal(r["inl"][f].astype(bool), o["inliers"])
        np.testing.assert_array_equal(r["pose"][f].view(np.uint64), o["pose"].view(np.uint64))
        np.testing.assert_allclose(r["rsum"][f], o["residual_sum"], rtol=1e-10)      # (a wave reduction sums in another order)
        po, oo = P.p3p_solve(x[f][samples[f // group]], X[samples[f // group]])
        np.testing.assert_array_equal(r["valid"][f], oo)
        np.testing.assert_array_equal(r["hyp"][f].view(np.uint64), po.view(np.uint64))
    assert set(np.unique(r["inl"])) <= {0, 1}


# H: no multiple of the 4 samples of a scoring workgroup nor of the 128 threads of the hypotheses kernel, fewer than 256
# scores in the select reduction; N: the minimum, and one more than a wavefront
@pytest.mark.parametrize("N,H", [(3, 1), (3, 3), (65, 1), (65, 3), (65, 5), (65, 129), (3, 129)])
def test_small_and_odd_shapes_match_oracle(N, H):
    F = 2
    X, x = scene(N, F, seed=100 * N + H)
    rng = np.random.default_rng(H)
    samples = draw(rng, F, H, N)
    thr = np.array([1e-6, 4e-6])
    r = run(x, X, None, samples, thr)
    check_against_oracle(r, x, X, None, samples, thr)
    if H == 129 and N == 65:
        assert (r["num"] > N // 2).all()


def test_two_virtual_frames_per_sample_set():
    N, H, group = 65, 5, 2
    X, x0 = scene(N, 2, seed=5)
    fac = np.array([0.8, 1.25])
    x = (x0[:, None] / fac[None, :, None, None]).reshape(4, N, 2)          # (frame, focal length factor)
    rng = np.random.default_rng(6)
    samples = draw(rng, 2, H, N)
    mask = rng.random((4, N)) < 0.9
    thr = np.full(4, 1e-6) * rng.uniform(0.5, 2.0, 4)
    r = run(x, X, mask, samples, thr, group)
    check_against_oracle(r, x, X, mask, samples, thr, group)


def test_frame_without_a_valid_sample_beside_good_frames():
    N, H = 65, 5
    X, x = scene(N, 3, seed=8)
    rng = np.random.default_rng(9)
    samples = draw(rng, 3, H, N)
    samples[1] = samples[1][:, :1]                                          # three times the same point: no triangle
    thr = np.full(3, 1e-6)
    r = run(x, X, None, samples, thr)
    check_against_oracle(r, x, X, None, samples, thr)
    assert not r["valid"][1].any() and r["num"][1] == 0 and r["best"][1] == -1
    assert not r["pose"][1].any() and not r["inl"][1].any() and r["rsum"][1] == 0.0
    assert r["num"][0] > N // 2 and r["num"][2] > N // 2


def test_masked_sample_point_still_makes_a_hypothesis():
    N = 10
    X, x = scene(N, 1, seed=12, outliers=0.0, noise=0.0)
    samples = np.array([[[0, 1, 2]]], np.int32)
    mask = np.ones((1, N), bool)
    mask[0, 1] = False
    thr = np.array([1e-12])
    r = run(x, X, mask, samples, thr)
    check_against_oracle(r, x, X, mask, samples, thr)
    assert r["num"][0] == N - 1 and not r["inl"][0, 1] and r["inl"][0].sum() == N - 1 and r["best"][0] >= 0


def _straddle(value_of, start, target, steps=8):
    """arguments a few ulps either side of the one at which value_of crosses target"""
    lo = hi = start
    for _ in range(200):                                                   # walk to the crossing
        if value_of(lo) > target:
            lo = np.nextafter(lo, -np.inf)
        elif value_of(hi) <= target:
            hi = np.nextafter(hi, np.inf)
        else:
            break
    out = [lo, hi]
    for _ in range(steps):
        out = [np.nextafter(out[0], -np.inf)] + out + [np.nextafter(out[-1], np.inf)]
    return np.array(out)


def test_points_on_the_threshold_and_on_the_depth_limit():
    # One sample; the scene has a pose of small integers, so X and x are short binary fractions and the solver's pose is the
    # integer one up to a few ulps.  Frame 0: a point whose squared error is the threshold itself, bit for bit, and the
    # neighbouring doubles either side of it; frame 1 (threshold 1e30: whatever is in front is an inlier): points whose depth
    # is as close to 1e-12 as the pose's ulps allow, either side.  One ulp of difference between the device and the oracle
    # moves a point across and changes a count.
    X3 = np.array([[0.5, -0.25, 1.0], [-0.75, 0.5, 2.0], [0.25, 0.75, -0.5]])
    Y3 = X3 @ INT_POSE[:, :3].T + INT_POSE[:, 3]
    x3 = Y3[:, :2] / Y3[:, 2:]
    poses, ok = P.p3p_solve(x3[None], X3[None])
    k = int(np.argmin(np.where(ok[0], np.abs(poses[0] - INT_POSE).max((-1, -2)), np.inf)))
    Pm = poses[0, k]
    assert ok[0, k] and np.abs(Pm - INT_POSE).max() < 1e-12

    def point(Xp):                                                         # as point_error / score_poses compute it
        return [((Pm[i, 0] * Xp[0] + Pm[i, 1] * Xp[1]) + Pm[i, 2] * Xp[2]) + Pm[i, 3] for i in range(3)]

    Xa = np.array([0.25, 0.5, 1.0])
    pa = point(Xa)
    ua, wa = pa[0] / pa[2], pa[1] / pa[2]

    def err(u):
        ex, ey = ua - u, wa - wa
        return ex * ex + ey * ey
    us = _straddle(lambda u: -err(u), ua - 0.03125, -0.0009765625)         # err falls as u rises towards the projection
    thr = err(us[len(us) // 2])                                            # ~2^-10, and exactly the error of one point
    zs = _straddle(lambda z: point([0.25, 0.5, z])[2], 1e-12 - Pm[2, 3], 1e-12)
    na, nz = len(us), len(zs)
    X = np.concatenate([X3, np.tile(Xa, (na, 1)), np.stack([np.full(nz, 0.25), np.full(nz, 0.5), zs], 1)])
    x = np.zeros((2, len(X), 2))
    x[:, :3] = x3
    x[:, 3:3 + na, 0], x[:, 3:3 + na, 1] = us, wa
    samples = np.array([[[0, 1, 2]]], np.int32)
    thr_sq = np.array([thr, 1e30])
    # the cases are what they claim to be: under solution k one point sits on the threshold, others either side of it, and
    # the depths lie either side of 1e-12
    ea = np.array([err(u) for u in us])
    depth = np.array([point(Xz)[2] for Xz in X[3 + na:]])
    assert (ea == thr).any() and (ea < thr).any() and (ea > thr).any() and (depth > 1e-12).any() and (depth <= 1e-12).any()
    assert np.abs(depth - 1e-12).min() < 1e-15
    cnt, _, inl = P.score_poses(poses[0], x[0], X, np.ones(len(X), bool), thr)
    np.testing.assert_array_equal(inl[k, 3:3 + na], ea <= thr)
    _, _, inl1 = P.score_poses(poses[0], x[1], X, np.ones(len(X), bool), 1e30)
    np.testing.assert_array_equal(inl1[k, 3 + na:], depth > 1e-12)
    r = run(x, X, None, samples, thr_sq, group=2)
    check_against_oracle(r, x, X, None, samples, thr_sq, group=2)
    assert r["best"][0] == k                                               # frame 0 is won by the integer pose
    np.testing.assert_array_equal(r["inl"][0, 3:3 + na].astype(bool), ea <= thr)
    if r["best"][1] == k:
        np.testing.assert_array_equal(r["inl"][1, 3 + na:].astype(bool), depth > 1e-12)
