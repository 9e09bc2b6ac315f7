"""5-point essential-matrix LO-RANSAC on the GPU (csrc/essential.hip): the minimal solver against the independent CPU
solver of tests/essential_cases.py, degenerate samples, the whole flow against the reference's flow
(tests/golden/essential_flow_*.npz, scripts/make_golden_essential.py) and the properties of the production configuration.

Bounds (tests/essential_cases.py): SOLVER_BOUND is one decade above the largest deviation from the CPU solver measured on
an MI355X, FLOW_BOUND ten times that (local optimisation adds a 9x9 eigen-solve), POSE_BOUND one decade above the measured
angular errors; CONSTRAINT_BOUND 1e-8 is what a float64 solve of a well-conditioned sample satisfies, whatever was
measured.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from tests import essential_cases as EC
from vggsfm_amd import _lib
from vggsfm_amd.two_view_geo import essential as ES
from vggsfm_amd.two_view_geo import estimate_essential, relative_pose_from_essential, run_5point

pytestmark = pytest.mark.gpu


def D(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def five_point(p1, p2, samples):
    """(B,N,2) normalised, (H,5) -> candidates (B,H,10,3,3), flags (B,H,10) on the host"""
    E, ok = ES._five_point(_lib.lib(), D(p1, torch.float64), D(p2, torch.float64), D(samples, torch.int32))
    B, H = p1.shape[0], len(samples)
    return E.cpu().numpy().reshape(B, H, 10, 3, 3), ok.cpu().numpy().reshape(B, H, 10).astype(bool)


def assert_clean(E, ok):
    """finite or flagged: never a non-finite number in a valid slot, zeros in the others"""
    assert np.isfinite(E[ok]).all()
    assert (E[~ok] == 0).all()
    if ok.any():
        np.testing.assert_allclose(np.linalg.norm(E[ok], axis=(-2, -1)), 1.0, rtol=0, atol=1e-12)
    first_invalid = np.where(ok.all(-1), 10, np.argmin(ok, -1))       # valid slots come first
    assert (ok.sum(-1) == first_invalid).all()


# --- 1 ------------------------------------------------------------------------------------------------------------------
def test_minimal_solver_equals_the_cpu_solver():
    g = EC.load("solver")
    p1, p2, smp = g["points1"], g["points2"], g["samples"]
    E, ok = five_point(p1, p2, smp)
    assert_clean(E, ok)
    admit = g["admit_sample"]
    assert 1.0 - admit.mean() <= EC.CAP
    dev, cons, wrong_count = 0.0, np.zeros(3), []
    for b, h in zip(*np.nonzero(admit)):
        got, ref = E[b, h][ok[b, h]], g["cpu_emat"][b, h, :g["cpu_num"][b, h]]
        if len(got) != len(ref):
            wrong_count.append((b, h, len(got), len(ref)))
            continue
        dev = max(dev, EC.set_deviation(got, ref))
        for e in got:
            cons = np.maximum(cons, EC.constraint_residuals(e, p1[b, smp[h]], p2[b, smp[h]]))
    print(f"solver: {admit.sum()} admitted samples, {ok[admit].sum()} candidates; largest deviation from the CPU solver "
          f"{dev:.3e} (bound {EC.SOLVER_BOUND:.0e}); constraints: epipolar {cons[0]:.3e}, det {cons[1]:.3e}, "
          f"trace {cons[2]:.3e} (bound {EC.CONSTRAINT_BOUND:.0e}); samples with another number of real roots: {wrong_count}")
    assert not wrong_count
    assert cons.max() <= EC.CONSTRAINT_BOUND
    assert dev <= EC.SOLVER_BOUND


# --- 2 ------------------------------------------------------------------------------------------------------------------
def _edge_scene():
    """N = 8: matches 0..4 are images of coplanar points, 5..7 general"""
    rng = np.random.default_rng(5)
    R, t = EC.rodrigues(np.array([0.1, -0.2, 0.05])), np.array([0.6, 0.1, 0.2])
    X = np.stack([rng.uniform(-2, 2, 8), rng.uniform(-2, 2, 8), rng.uniform(4, 9, 8)], 1)
    X[:5, 2] = 6.0 + 0.3 * X[:5, 0] - 0.2 * X[:5, 1]
    Y = X @ R.T + t
    return (X[:, :2] / X[:, 2:])[None], (Y[:, :2] / Y[:, 2:])[None]


def test_degenerate_samples_are_finite_or_flagged():
    p1, p2 = _edge_scene()
    smp = np.array([[0, 1, 2, 3, 4],          # coplanar
                    [5, 6, 7, 5, 0],          # a repeated index
                    [5, 5, 5, 5, 5],          # one point five times
                    [0, 1, 2, 3, 8],          # out of range: flagged, not read
                    [-1, 1, 2, 3, 4],
                    [1, 2, 5, 6, 7]], np.int32)
    E, ok = five_point(p1, p2, smp)
    print("valid candidates per edge sample:", ok.sum(-1)[0])
    assert_clean(E, ok)
    assert not ok[0, 3].any() and not ok[0, 4].any()
    assert ok[0, 5].any()
    for h in (0, 5):                           # what a degenerate sample does return still fits its points
        for e in E[0, h][ok[0, h]]:
            assert EC.constraint_residuals(e, p1[0, smp[h]], p2[0, smp[h]])[0] <= 1e-6
    # a group past the end of the table (H = 6 is not a multiple of four) stores nothing: checked by the poison test


def test_two_real_roots_and_five_matches_exactly():
    """N = 5: the five matches of a golden sample whose polynomial has exactly two real roots"""
    g = EC.load("solver")
    two = np.argwhere((g["cpu_num"] == 2) & g["admit_sample"])
    assert len(two) > 0, "essential_solver.npz holds no admitted sample with exactly two real solutions"
    b, h = two[0]
    idx = g["samples"][h]
    p1, p2 = g["points1"][b, idx][None], g["points2"][b, idx][None]
    E, ok = five_point(p1, p2, np.array([[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]], np.int32))
    assert_clean(E, ok)
    assert (ok.sum(-1) == 2).all()
    dev = max(EC.set_deviation(E[0, k][ok[0, k]], g["cpu_emat"][b, h, :2]) for k in range(2))
    print(f"two real roots: deviation {dev:.3e}")
    assert dev <= EC.SOLVER_BOUND
    # the public function on the same five matches: identity in the unused slots
    full, flags = run_5point(D(p1), D(p2), return_valid=True)
    full, flags = full.cpu().numpy(), flags.cpu().numpy()
    assert full.shape == (1, 10, 3, 3) and flags.sum() == 2 and (full[0, 2:] == np.eye(3)).all()
    assert EC.set_deviation(full[0, :2], g["cpu_emat"][b, h, :2]) <= EC.FLOW_BOUND


def _refine_one(p1, p2, E_src, thr):
    L = _lib.lib()
    cnt = torch.tensor([[5]], dtype=torch.int32).cuda()
    order = torch.zeros((1, 1), dtype=torch.int32).cuda()
    E, ok = ES._refine(L, D(p1[None]), D(p2[None]), D(E_src.reshape(1, 1, 9)), cnt, order, D(np.array([thr])))
    return E.cpu().numpy().reshape(10, 3, 3), ok.cpu().numpy().reshape(10).astype(bool)


def test_local_optimisation_needs_five_inliers():
    rng = np.random.default_rng(9)
    f, pp = np.ones(4), np.zeros(4)
    p1, p2, R, t, _ = EC.two_view_scene(rng, 12, f, pp)
    Et = EC.true_essential(R, t)
    for inliers in (5, 4):
        q2 = p2.copy()
        q2[inliers:] += 0.3 + 0.2 * rng.uniform(size=(12 - inliers, 2))          # gross outliers
        assert (EC.sampson_sq(Et, p1, q2) <= 1e-12).sum() == inliers
        E, ok = _refine_one(p1, q2, Et, 1e-12)
        assert_clean(E[None], ok[None])
        print(f"local optimisation on {inliers} inliers: {ok.sum()} candidates")
        if inliers == 4:
            assert not ok.any()
        else:
            ref = EC.five_point(p1[:5], q2[:5])
            assert ok.sum() == len(ref) and EC.set_deviation(E[ok], ref) <= EC.FLOW_BOUND
            assert EC.distance(E[ok], Et).min() <= EC.FLOW_BOUND


def test_run_5point_on_many_masked_matches():
    """N = 300 (more than one sweep of the workgroup), the outliers masked out: the true E is among the candidates"""
    rng = np.random.default_rng(11)
    f, pp = np.ones(4), np.zeros(4)
    scenes = [EC.two_view_scene(rng, 300, f, pp, outliers=0.3) for _ in range(2)]
    p1, p2 = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    mask = np.stack([s[4] for s in scenes])
    E, ok = run_5point(D(p1), D(p2), masks=D(mask), return_valid=True)
    E, ok = E.cpu().numpy(), ok.cpu().numpy()
    assert (E[~ok] == np.eye(3)).all() and np.isfinite(E).all()
    for b in range(2):
        d = EC.distance(E[b][ok[b]], EC.true_essential(scenes[b][2], scenes[b][3])).min()
        ref = EC.five_point(p1[b], p2[b], mask[b].astype(np.float64))
        print(f"run_5point pair {b}: {ok[b].sum()} candidates (CPU {len(ref)}), true E within {d:.3e}")
        assert d <= EC.FLOW_BOUND and ok[b].sum() == len(ref)
    with pytest.raises(NotImplementedError):
        run_5point(D(p1), D(p2), weights=D(mask))


# --- 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.FLOW_CASES)
def test_whole_flow_equals_the_reference_flow(name):
    g = EC.load(name)
    assert g["admit_pair"].all() and 1.0 - g["admit_match"].mean() <= EC.CAP
    E, num, mask, res = estimate_essential(D(g["points1"]), D(g["points2"]), D(g["focal_length"]), D(g["principal_point"]),
                                           max_ransac_iters=len(g["samples"]), max_error=float(g["max_error"]),
                                           lo_num=int(g["lo_num"]), samples=g["samples"], return_residuals=True)
    assert E.dtype == torch.float64 and res.dtype == torch.float64 and mask.dtype == torch.bool
    E, num, mask, res = E.cpu().numpy(), num.cpu().numpy(), mask.cpu().numpy(), res.cpu().numpy()
    dev = EC.distance(E, g["ref_emat"])
    admit = g["admit_match"]
    print(f"{name}: winner deviation per pair {dev} (bound {EC.FLOW_BOUND:.0e}); inliers {num} (reference "
          f"{g['ref_inlier_num']}); masks differ on {(mask != g['ref_inlier_mask'])[admit].sum()} admitted matches")
    np.testing.assert_allclose(np.linalg.norm(E, axis=(-2, -1)), 1.0, rtol=0, atol=1e-12)
    assert (dev <= EC.FLOW_BOUND).all()
    assert (mask == g["ref_inlier_mask"])[admit].all()
    assert (np.abs(num - g["ref_inlier_num"]) <= (~admit).sum(1)).all()
    assert (num == mask.sum(1)).all()


# --- 4 ------------------------------------------------------------------------------------------------------------------
def _production():
    rng = np.random.default_rng(21)
    B, N, H = 4, 200, 256
    focal = np.array([[900.0, 900, 900, 900], [1100, 1050, 700, 720], [500, 500, 1500, 1500], [800, 820, 790, 805]])
    pp = rng.uniform(300, 600, (B, 4))
    scenes = [EC.two_view_scene(rng, N, focal[b], pp[b], outliers=0.3, outlier_clearance=20.0) for b in range(B)]
    samples = np.array([rng.choice(N, 5, replace=False) for _ in range(H)], np.int32)
    samples[0] = np.arange(N - 5, N)                                  # all inliers (the outliers come first)
    return scenes, focal, pp, samples


def test_production_configuration():
    scenes, focal, pp, samples = _production()
    px1, px2 = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    args = dict(max_ransac_iters=len(samples), max_error=4, lo_num=50, samples=samples, return_residuals=True)
    run = lambda sl: [x.cpu().numpy() for x in estimate_essential(D(px1[sl]), D(px2[sl]), D(focal[sl]), D(pp[sl]), **args)]
    E, num, mask, res = run(slice(None))
    thr = (4.0 / focal.mean(1)) ** 2
    assert np.array_equal(mask, res <= thr[:, None]) and np.array_equal(num, mask.sum(1))
    again = run(slice(None))
    assert all(same_bits(a, b) for a, b in zip((E, num, mask, res), again)), "two runs differ"
    for b in range(len(scenes)):
        alone = run(slice(b, b + 1))
        assert all(same_bits(a[b:b + 1], c) for a, c in zip((E, num, mask, res), alone)), f"pair {b} alone differs"
    # lo_num = 0: no local optimisation (the reference's meaning); the winner is then one of the RANSAC candidates
    E0, num0, mask0 = [x.cpu().numpy() for x in estimate_essential(D(px1), D(px2), D(focal), D(pp), max_error=4, lo_num=0,
                                                                   samples=samples)]
    assert np.array_equal(num0, mask0.sum(1)) and (num0 <= num).all() and np.isfinite(E0).all()
    true_inliers = np.array([s[4].sum() for s in scenes])
    print(f"production: inliers {num}, true inliers {true_inliers}")
    assert (num >= true_inliers).all()        # (no outlier lies within 20 px of its epipolar line: equality)
    R, t = relative_pose_from_essential(D(E), D(px1), D(px2), D(focal), D(pp))
    R, t = R.cpu().numpy(), t.cpu().numpy()
    rot = [2 * np.arcsin(min(1.0, np.linalg.norm(R[b] - s[2]) / (2 * np.sqrt(2)))) for b, s in enumerate(scenes)]
    tra = [np.arctan2(np.linalg.norm(np.cross(t[b], s[3])), abs(t[b] @ s[3])) for b, s in enumerate(scenes)]
    print(f"production: rotation errors {np.array(rot)} rad, translation direction errors {np.array(tra)} rad "
          f"(bound {EC.POSE_BOUND:.0e}); E deviation {[EC.distance(E[b], EC.true_essential(s[2], s[3])) for b, s in enumerate(scenes)]}")
    assert max(rot) <= EC.POSE_BOUND and max(tra) <= EC.POSE_BOUND
