"""CPU, only where /root/reference exists: the pieces of the two-view oracle that CAN be pinned against the reference's
own code.  vggsfm/two_view_geo imports kornia at module level (absent here: the import harness fabricates it), so the
reference functions run with kornia's five trivial helpers restated below (homogeneous padding, a 3x3 transform of
points, division by F[2,2], and aliases of torch.cat / stack / ones_like / zeros / where); what is compared is the
reference's OWN arithmetic:

    sampson_epipolar_distance_batched (utils.py:90-172, float32)   vs  oracle sampson_sq
    run_8point + normalize_points_masked (fundamental.py:261-334, utils.py:175-253)  vs  oracle eight_point
    local_refinement's mask gathering (utils.py:256-298)            vs  the oracle's selection of inlier sets
    calculate_residual_indicator + argmax (utils.py:63-87, fundamental.py:162-176)   vs  oracle _best

    run_7point (fundamental.py:341-469, float32) with kornia's normalize_points restated and the roots of ITS cubic
      coefficients taken with numpy.roots                           vs  oracle seven_point

Not pinnable here: kornia's own solve_cubic (third-party, kornia is not in this image: its closed-form root finder is
replaced by numpy.roots on the coefficients the reference computes) and the sampling RNG."""
import numpy as np
import pytest
import torch

from oracle import fundamental as Fd
from oracle import ref_replay
from tests.test_oracle_fundamental import two_view

REF = ref_replay.calls("oracle_fundamental_vs_reference")


def _reference_modules():
    rf = REF.module("vggsfm.two_view_geo.fundamental")
    ru = REF.module("vggsfm.two_view_geo.utils")

    def to_h(p):
        return torch.cat([p, torch.ones_like(p[..., :1])], -1)

    def transform_points(T, p):                       # kornia.geometry.linalg.transform_points for affine 3x3 T
        q = to_h(p) @ T.transpose(-2, -1)
        return q[..., :2] / q[..., 2:]

    def normalize_transformation(M, eps=1e-8):        # kornia.geometry.epipolar.normalize_transformation
        nv = M[..., -1:, -1:]
        return torch.where(nv.abs() > eps, M / (nv + eps), M)
    for mod in (rf, ru):
        mod.ones_like, mod.stack, mod.zeros, mod.where, mod.concatenate = torch.ones_like, torch.stack, torch.zeros, torch.where, torch.cat
        mod.normalize_transformation = normalize_transformation
        mod.Tensor = torch.Tensor                     # (kornia.core.Tensor is torch.Tensor)
    ru.convert_points_to_homogeneous = to_h
    ru.transform_points = transform_points
    return rf, ru


def _unit(F):
    F = F / np.linalg.norm(F, axis=(-2, -1), keepdims=True)
    return F * np.sign(F[..., 2, 2])[..., None, None]


def test_sampson_distance_matches_reference():
    rf, ru = _reference_modules()
    x1, x2, _, Ft = two_view(500, 4)
    rng = np.random.default_rng(0)
    F = np.stack([Ft + 0.02 * rng.normal(size=(3, 3)) * np.abs(Ft).max() for _ in range(6)])
    ref = ru.sampson_epipolar_distance_batched(torch.from_numpy(x1).float()[None], torch.from_numpy(x2).float()[None],
                                               torch.from_numpy(F).float()[None], squared=True)[0].double().numpy()
    mine = Fd.sampson_sq(F, x1, x2)
    np.testing.assert_allclose(mine, ref, rtol=2e-2, atol=1e-3)                     # (the reference computes in float32)
    assert np.median(np.abs(mine - ref) / (np.abs(ref) + 1e-6)) < 1e-4


def test_eight_point_and_mask_gathering_match_reference():
    rf, ru = _reference_modules()
    x1, x2, out, Ft = two_view(800, 6)
    rng = np.random.default_rng(1)
    K, lo = 12, 5
    inl = rng.random((K, 800)) < 0.7
    inl[:, out] = False
    order = Fd._order(inl.sum(1).astype(np.int64))                                   # stable descending, like torch.sort
    t1, t2 = torch.from_numpy(x1)[None], torch.from_numpy(x2)[None]
    ref = ru.local_refinement(rf.run_8point, t1, t2, torch.from_numpy(inl)[None], torch.from_numpy(order)[None], lo_num=lo)
    ref = ref[0].numpy()                                                              # (lo,3,3), scaled to F[2,2] = 1
    mine, ok = Fd.eight_point(x1, x2, inl[order[:lo]])
    assert ok.all()
    np.testing.assert_allclose(_unit(mine), _unit(ref), atol=2e-8)
    # both enforce rank 2 and describe the scene
    assert np.abs(np.linalg.det(_unit(ref))).max() < 1e-12 and np.abs(np.linalg.det(mine)).max() < 1e-12
    assert np.abs(_unit(mine) - _unit(Ft[None])).max() < 5e-3


def test_winner_selection_matches_reference():
    rf, ru = _reference_modules()
    rng = np.random.default_rng(2)
    for trial in range(20):
        B, K, N, thr = 3, 40, 60, 1.0
        res = rng.uniform(0, 3, size=(B, K, N))
        res[:, rng.integers(0, K, 5)] = 7.0                                          # hypotheses without inliers
        res[:, 3] = res[:, 1]                                                        # an exact tie: the first wins
        ind, num, mask = ru.calculate_residual_indicator(torch.from_numpy(res), thr)
        ref_best = torch.argmax(ind, dim=1).numpy()
        for b in range(B):
            inl = res[b] <= thr
            cnt = inl.sum(1).astype(np.int64)
            rs = np.where(inl, res[b], 0.0).sum(1)
            assert Fd._best(cnt, rs) == ref_best[b]
            assert np.array_equal(num[b].numpy(), cnt) and np.array_equal(mask[b].numpy(), inl)


def test_residual_indicator_mirror_equals_reference():
    """vggsfm_amd.two_view_geo.utils.calculate_residual_indicator (plain tensor ops) = the reference's function, bit for
    bit (same operations in the same order)."""
    rf, ru = _reference_modules()
    from vggsfm_amd.two_view_geo.utils import calculate_residual_indicator
    rng = np.random.default_rng(5)
    for trial in range(10):
        res = torch.from_numpy(rng.uniform(0, 3, size=(2, 17, 50)))
        res[:, 4] = 9.0                                                              # a hypothesis without inliers
        a = calculate_residual_indicator(res, 1.0)
        b = ru.calculate_residual_indicator(res, 1.0)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_depth_helper_mirror_equals_reference():
    """vggsfm_amd.two_view_geo.utils.calculate_depth_batch = the reference's (triangulation.py imports it), bit for bit."""
    rf, ru = _reference_modules()
    from vggsfm_amd.two_view_geo.utils import calculate_depth_batch
    rng = np.random.default_rng(6)
    P = torch.from_numpy(rng.normal(size=(4, 3, 4)))
    X = torch.from_numpy(rng.normal(size=(4, 33, 3)))
    assert torch.equal(calculate_depth_batch(P, X), ru.calculate_depth_batch(P, X))


def test_seven_point_pencil_matches_reference_modulo_the_cubic_solver():
    """run_7point (fundamental.py:339-469) with kornia's normalize_points restated and its solve_cubic replaced by
    numpy.roots (real roots, zeros elsewhere): the null-space pencil, the cubic's coefficients, the F[2,2] = 1 scaling and
    the de-normalisation are the reference's own arithmetic.  Every matrix the oracle reports must be one of the
    reference's (the reference also emits a junk matrix per non-real root, which the oracle flags invalid instead)."""
    rf, ru = _reference_modules()

    def normalize_points(points, eps=1e-8):           # kornia.geometry.epipolar.normalize_points
        mean = points.mean(-2, keepdim=True)
        scale = (points - mean).norm(dim=-1, p=2).mean(-1)
        scale = torch.sqrt(torch.tensor(2.0)) / (scale + eps)
        o, z = torch.ones_like(scale), torch.zeros_like(scale)
        T = torch.stack([scale, z, -scale * mean[..., 0, 0], z, scale, -scale * mean[..., 0, 1], z, z, o], -1).view(-1, 3, 3)
        return ru.transform_points(T, points), T

    def solve_cubic(coeffs):
        out = torch.zeros(coeffs.shape[0], 3, dtype=coeffs.dtype)
        for i, c in enumerate(coeffs.numpy()):
            r = np.roots(c)
            r = np.sort(r[np.abs(r.imag) < 1e-10].real)
            out[i, :len(r)] = torch.from_numpy(r)
        return out
    rf.normalize_points, rf.solve_cubic = normalize_points, solve_cubic
    rf.KORNIA_CHECK_SHAPE = lambda *a, **k: None
    x1, x2, _, Ft = two_view(400, 8, outliers=0.0, noise=0.2)
    rng = np.random.default_rng(3)
    smp = np.stack([rng.choice(400, 7, replace=False) for _ in range(150)])
    # (the reference's last assignment casts to float32, so the function only runs in float32)
    ref = rf.run_7point(torch.from_numpy(x1[smp]).float(), torch.from_numpy(x2[smp]).float()).double().numpy()   # (150,3,3,3)
    mine, ok = Fd.seven_point(x1[smp], x2[smp])
    assert ok.any(1).all()
    ru_ = _unit(ref)
    dist = []
    for h in range(150):
        for s in range(3):
            if ok[h, s]:
                dist.append(np.abs(ru_[h] - _unit(mine[h, s])[None]).max((-1, -2)).min())
    dist = np.array(dist)
    assert len(dist) >= 150 and np.median(dist) < 1e-4 and (dist < 5e-3).mean() > 0.97, (np.median(dist), np.sort(dist)[-8:])


def test_preliminary_camera_helpers_match_reference():
    """``essential_from_fundamental``, ``decompose_essential_matrix``, ``build_default_kmat`` of
    vggsfm_amd/two_view_geo/estimate_preliminary.py (torch ops, device agnostic) against the reference's own functions
    (vggsfm/two_view_geo/fundamental.py:186-212, essential.py:36-83 -- kornia's ``cross_product_matrix`` / ``eye_like``
    style helpers restated by the harness -- and estimate_preliminary.py:244-272)."""
    import torch
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        RE = REF.module("vggsfm.two_view_geo.essential")
        RP = REF.module("vggsfm.two_view_geo.estimate_preliminary")
        RF = REF.module("vggsfm.two_view_geo.fundamental")
    from vggsfm_amd.two_view_geo import estimate_preliminary as P
    # kornia helpers the reference imports by name (stubbed by the harness): restated here
    RE.ones_like, RE.where, RE.stack = torch.ones_like, torch.where, torch.stack
    RE._torch_svd_cast = lambda m: torch.svd(m)

    def cross_product_matrix(x):
        x0, x1, x2 = x[..., 0], x[..., 1], x[..., 2]
        z = torch.zeros_like(x0)
        return torch.stack([z, -x2, x1, x2, z, -x0, -x1, x0, z], dim=-1).view(*x.shape[:-1], 3, 3)
    RE.cross_product_matrix = cross_product_matrix
    rng = np.random.default_rng(3)
    from scipy.spatial.transform import Rotation
    B = 7
    Rt = Rotation.random(B, random_state=2).as_matrix()
    tt = rng.normal(size=(B, 3))
    tt /= np.linalg.norm(tt, axis=1, keepdims=True)
    tx = np.zeros((B, 3, 3))
    tx[:, 0, 1], tx[:, 0, 2], tx[:, 1, 0], tx[:, 1, 2], tx[:, 2, 0], tx[:, 2, 1] = -tt[:, 2], tt[:, 1], tt[:, 2], -tt[:, 0], -tt[:, 1], tt[:, 0]
    E = torch.from_numpy(tx @ Rt)
    k1r, k2r, flr, ppr = RP.build_default_kmat(1024, 768, 1, B + 1, 10, device="cpu", dtype=torch.float64)
    k1, k2, fl, pp = P.build_default_kmat(1024, 768, 1, B + 1, 10, device="cpu", dtype=torch.float64)
    for a, b in ((k1, k1r), (k2, k2r), (fl, flr), (pp, ppr)):
        assert torch.equal(a, b)
    F = torch.linalg.inv(k2).transpose(-2, -1) @ E @ torch.linalg.inv(k1)
    Er, _, _ = RF.essential_from_fundamental(F, k1, k2)
    Em = P.essential_from_fundamental(F, k1, k2)
    assert torch.allclose(Em, Er, rtol=0, atol=1e-12) and torch.allclose(Em, E, atol=1e-9)
    Rs_r, Ts_r = RE.decompose_essential_matrix(E)
    Rs, Ts = P.decompose_essential_matrix(E)
    # the candidate SET is what matters (an SVD is unique up to joint sign flips): every reference candidate is among ours
    for b in range(B):
        for c in range(4):
            d = [(Rs[b, k] - Rs_r[b, c]).abs().max().item() + (Ts[b, k] - Ts_r[b, c]).abs().max().item() for k in range(4)]
            assert min(d) < 1e-9
        # and the true motion is one of them (t up to sign is handled by the +-t pair)
        d = [np.abs(Rs[b, k].numpy() - Rt[b]).max() + np.abs(Ts[b, k].numpy() - tt[b]).max() for k in range(4)]
        assert min(d) < 1e-8
