"""The Sim(3) and pose-error kernels (csrc/sim3.hip, vggs_*) against the long-double yardstick of tests/sim3_cases.py.

The bound on every floating-point comparison is the rule of tests/test_gpu_covariance.py: max(1e-12, 100 x the deviation
of a float64 numpy evaluation of the same quantity from the same long-double reference).  Counts and masks are compared
exactly and nothing is left out: tests/test_sim3_reference.py asserts that no residual of these cases lies within 1e-9
max_error^2 of its threshold.

Measured on an MI355X, GPU deviation / float64 numpy deviation / bound, the component (ds, dR, dt) nearest its bound:
    n3                      3.0e-16 / 3.5e-16 / 1.0e-12      n4_one_masked           4.1e-16 / 5.2e-16 / 1.0e-12
    n63                     3.3e-16 / 4.1e-16 / 1.0e-12      n64                     3.3e-16 / 3.7e-16 / 1.0e-12
    n65                     4.7e-16 / 3.4e-16 / 1.0e-12      n257                    3.9e-16 / 3.9e-16 / 1.0e-12
    n5000_multi_workgroup   3.3e-16 / 4.0e-16 / 1.0e-12      b3_masks                3.1e-16 / 2.5e-16 / 1.0e-12
    float_weights           3.2e-16 / 3.1e-16 / 1.0e-12      no_scale                3.1e-16 / 8.6e-16 / 1.0e-12
    scale_1e-3_offset_1e4   2.4e-16 / 9.2e-16 / 1.0e-12      scale_1e3_offset_1e4    9.8e-14 / 1.3e-12 / 1.3e-10
    n5000_offset_1e4        1.0e-15 / 5.8e-15 / 1.0e-12      reflection              1.2e-16 / 2.8e-16 / 1.0e-12
    planar                  3.0e-16 / 1.7e-16 / 1.0e-12
    residual sums (relative)  H = 1: 3.0e-15 / 1.3e-15 / 1.0e-12   31: 3.1e-14 / 3.1e-14 / 3.1e-12   32: 2.7e-14 / 2.5e-14 /
                              2.5e-12   33: 1.5e-14 / 1.3e-14 / 1.3e-12
    ransac, final transforms  7.1e-16 / 8.6e-16 / 1.0e-12 at the worst
    pair errors (degrees)     S = 2: 6.3e-14 / 6.3e-14 / 6.3e-12   S = 7: 1.3e-12 / 4.1e-13 / 4.1e-11   S = 65: 1.8e-11 /
                              1.3e-11 / 1.3e-09
Every test prints its figures before it asserts.
"""
import copy

import numpy as np
import pytest
import torch

from tests import sim3_cases as SC
from vggsfm_amd import _lib, sim3
from vggsfm_amd import pycolmap_compat as pc
from vggsfm_amd.scene import make_scene
from vggsfm_amd.utils import metric

pytestmark = pytest.mark.gpu
LD = np.longdouble
FIT = SC.fit_cases()


def _dev(a, dtype=torch.float64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


def _bound(f64_dev):
    return max(1e-12, 100.0 * f64_dev)


def _fit(c):
    s, R, t, ok = sim3.estimate_sim3(_dev(c["src"]), _dev(c["tgt"]), _dev(c["weights"]), c["estimate_scale"])
    return s.cpu().numpy(), R.cpu().numpy(), t.cpu().numpy(), ok.cpu().numpy()


# --- fit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, c in FIT.items() if c["valid"]])
def test_fit_against_the_long_double_reference(name):
    c = FIT[name]
    s, R, t, ok = _fit(c)
    assert ok.all() and ok.shape == (len(c["src"]),)
    for b in range(len(c["src"])):
        w = None if c["weights"] is None else c["weights"][b]
        ref = SC.umeyama(c["src"][b], c["tgt"][b], w, c["estimate_scale"])
        assert ref[3]
        got = SC.fit_deviation((s[b], R[b], t[b]), ref[:3], c["src"][b], w)
        f64 = SC.fit_deviation(SC.umeyama_f64(c["src"][b], c["tgt"][b], w, c["estimate_scale"]), ref[:3], c["src"][b], w)
        for what, g, f in zip(("ds", "dR", "dt"), got, f64):
            print(f"{name}[{b}] {what}: GPU {g:.2e} / float64 {f:.2e} / bound {_bound(f):.2e}")
        for g, f in zip(got, f64):
            assert g <= _bound(f)
        assert abs(np.linalg.det(R[b]) - 1) < 1e-12
        if not c["estimate_scale"]:
            assert s[b] == 1.0


@pytest.mark.parametrize("name", [n for n, c in FIT.items() if not c["valid"]])
def test_fit_flags_degenerate_sets_and_writes_the_identity(name):
    s, R, t, ok = _fit(FIT[name])
    assert not ok.any() and (s == 1).all() and (R == np.eye(3)).all() and (t == 0).all()


def test_fit_does_not_read_what_carries_no_weight_and_is_deterministic():
    c = FIT["b3_masks"]
    src, tgt = c["src"].copy(), c["tgt"].copy()
    src[c["weights"] == 0] = np.nan
    tgt[c["weights"] == 0] = np.inf
    a = _fit(c)
    b = _fit(dict(c, src=src, tgt=tgt))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    big = FIT["n5000_multi_workgroup"]
    for x, y in zip(_fit(big), _fit(big)):
        assert np.array_equal(x, y)
    # one problem's result does not depend on what else is in the launch
    alone = _fit(dict(c, src=c["src"][1:2], tgt=c["tgt"][1:2], weights=c["weights"][1:2]))
    for x, y in zip(a, alone):
        assert np.array_equal(x[1:2], y)
    # a single (N,3) problem comes back without the batch dimension
    s, R, t, ok = sim3.estimate_sim3(_dev(c["src"][0]), _dev(c["tgt"][0]))
    assert s.shape == () and R.shape == (3, 3) and t.shape == (3,) and ok.shape == () and bool(ok)


# --- score --------------------------------------------------------------------------------------------------------------
def _hypotheses(sc, mask=None):
    """The long-double minimal transforms of a case's samples as float64 arrays (B,H,...) and their validity."""
    B, H, _ = sc["samples"].shape
    s, R, t, ok = np.ones((B, H)), np.tile(np.eye(3), (B, H, 1, 1)), np.zeros((B, H, 3)), np.zeros((B, H), bool)
    for b in range(B):
        for h in range(H):
            out = SC.sample_transform(sc["src"][b], sc["tgt"][b], None if mask is None else mask[b], sc["samples"][b, h])
            s[b, h], R[b, h], t[b, h], ok[b, h] = (np.asarray(x, np.float64) for x in out)
    return s, R, t, ok


@pytest.mark.parametrize("H", [1, SC.SCORE_TILE - 1, SC.SCORE_TILE, SC.SCORE_TILE + 1])
def test_score_counts_equal_and_sums_within_the_bound(H):
    sc = SC.score_case(H)
    s, R, t, ok = _hypotheses(sc)
    args = (_dev(sc["src"]), _dev(sc["tgt"]), _dev(s), _dev(R), _dev(t), _dev(ok, torch.uint8), _dev(sc["max_error"]))
    counts, sums = (x.cpu().numpy() for x in sim3.score_sim3(*args))
    again = [x.cpu().numpy() for x in sim3.score_sim3(*args)]
    assert np.array_equal(counts, again[0]) and np.array_equal(sums.view(np.int64), again[1].view(np.int64))
    assert counts.shape == sums.shape == (2, H) and counts.dtype == np.int32
    worst = (0.0, 0.0)
    for b in range(2):
        for h in range(H):
            if not ok[b, h]:
                assert counts[b, h] == -1 and sums[b, h] == 0
                continue
            T = (s[b, h], R[b, h], t[b, h])                    # the float64 transform the device was given, scored in long double
            c_ref, s_ref, _, _ = SC.score(T, sc["src"][b], sc["tgt"][b], None, sc["max_error"][b])
            _, s_f64, _, _ = SC.score(T, sc["src"][b], sc["tgt"][b], None, sc["max_error"][b], np.float64)
            assert counts[b, h] == c_ref
            scale = max(float(s_ref), float(sc["max_error"][b]) ** 2)
            g, f = abs(float(sums[b, h] - s_ref)) / scale, abs(float(s_f64 - s_ref)) / scale
            assert g <= _bound(f)
            worst = max(worst, (g, f))
    print(f"H = {H}: residual sums: GPU {worst[0]:.2e} / float64 {worst[1]:.2e} / bound {_bound(worst[1]):.2e}")
    assert (counts.max(1) > 150).all() or H == 1


def test_score_respects_the_mask():
    sc = SC.score_case(SC.SCORE_TILE + 1)
    s, R, t, ok = _hypotheses(sc)
    mask = np.ones((2, 300), bool)
    mask[0, ::3] = False
    src = sc["src"].copy()
    src[~mask] = np.nan
    counts, _ = sim3.score_sim3(_dev(src), _dev(sc["tgt"]), _dev(s), _dev(R), _dev(t), _dev(ok, torch.uint8), _dev(sc["max_error"]),
                                mask=_dev(mask, torch.uint8))
    counts = counts.cpu().numpy()
    for b in range(2):
        for h in np.nonzero(ok[b])[0]:
            assert counts[b, h] == SC.score((s[b, h], R[b, h], t[b, h]), sc["src"][b], sc["tgt"][b], mask[b], sc["max_error"][b])[0]


# --- ransac -------------------------------------------------------------------------------------------------------------
def _ransac(sc, lo_rounds, **kw):
    out = sim3.estimate_sim3_robust(_dev(sc["src"]), _dev(sc["tgt"]), _dev(sc["max_error"]), mask=_dev(sc["mask"], torch.uint8),
                                    lo_rounds=lo_rounds, samples=sc["samples"], return_scores=True, **kw)
    torch.cuda.synchronize()
    flat = out[:6] + out[6] + out[7:]
    return [x.cpu().numpy() for x in flat]          # scale, R, t, num, inliers, success, counts, sums, best, rounds


@pytest.fixture(scope="module")
def ransac_runs():
    sc = SC.ransac_case()
    return sc, {lo: _ransac(sc, lo) for lo in (0, 1, 2, 3)}


def test_ransac_winner_is_the_winner_of_its_own_score_table(ransac_runs):
    sc, runs = ransac_runs
    s, R, t, num, inl, success, counts, sums, best, rounds = runs[0]
    assert success.all() and (rounds == 0).all() and counts.shape == (3, 128)
    for b in range(3):
        assert best[b] == SC.rank_best(counts[b], sums[b])
        assert num[b] == counts[b, best[b]] == inl[b].sum()
        ref = SC.sample_transform(sc["src"][b], sc["tgt"][b], sc["mask"][b], sc["samples"][b, best[b]])
        # lo_rounds = 0: the minimal winner as it is; its counts are the reference's for every hypothesis
        got = SC.fit_deviation((s[b], R[b], t[b]), ref[:3], sc["src"][b][sc["samples"][b, best[b]]])
        f64 = SC.fit_deviation(SC.umeyama_f64(sc["src"][b][sc["samples"][b, best[b]]], sc["tgt"][b][sc["samples"][b, best[b]]]),
                               ref[:3], sc["src"][b][sc["samples"][b, best[b]]])
        print(f"problem {b} minimal winner {best[b]}: GPU {max(got):.2e} / float64 {max(f64):.2e} / bound {_bound(max(f64)):.2e}")
        for g, f in zip(got, f64):
            assert g <= _bound(f)
        for h in range(128):
            T = SC.sample_transform(sc["src"][b], sc["tgt"][b], sc["mask"][b], sc["samples"][b, h])
            want = SC.score(T[:3], sc["src"][b], sc["tgt"][b], sc["mask"][b], sc["max_error"][b])[0] if T[3] else -1
            assert counts[b, h] == want, (b, h)
        assert (counts[b] < 0).any()
    for lo in (1, 2, 3):                                    # the score table is that of the minimal hypotheses, whatever LO does
        assert np.array_equal(runs[lo][6], counts) and np.array_equal(runs[lo][7], sums) and np.array_equal(runs[lo][8], best)


def test_ransac_lo_follows_the_reference_round_by_round(ransac_runs):
    sc, runs = ransac_runs
    best = runs[0][8]
    for b in range(3):
        src, tgt, mask, err = sc["src"][b], sc["tgt"][b], sc["mask"][b], sc["max_error"][b]
        T0 = SC.sample_transform(src, tgt, mask, sc["samples"][b, best[b]])[:3]
        for lo in (0, 1, 2, 3):
            T, count, rsum, inl, accepted, _ = SC.local_optimisation(T0, src, tgt, mask, err, lo)
            s, R, t, num, got_inl, success, _, _, _, rounds = runs[lo]
            assert rounds[b] == accepted and num[b] == count and np.array_equal(got_inl[b], inl), (b, lo)
            if lo == 3:
                w = inl.astype(np.float64)
                got = SC.fit_deviation((s[b], R[b], t[b]), T, src, w)
                f64 = SC.fit_deviation(SC.umeyama_f64(src, tgt, w), T, src, w) if accepted else (0.0, 0.0, 0.0)
                print(f"problem {b}: {accepted} accepted rounds, {count} inliers; final transform: GPU {max(got):.2e} / "
                      f"float64 {max(f64):.2e} / bound {_bound(max(f64)):.2e}")
                for g, f in zip(got, f64):
                    assert g <= _bound(f)
                for e, bound in SC.recovery((s[b], R[b], t[b]), sc["truth"][b], src, inl, sc["sigma"]):
                    assert e <= bound
    assert runs[3][9][2] >= 2                               # problem 2 needed more than one round


def test_ransac_failures_replay_and_determinism():
    sc = SC.ransac_case()
    hard = copy.deepcopy(sc)
    hard["samples"][0, :, 1] = hard["samples"][0, :, 0]     # problem 0: every sample degenerate
    hard["mask"][1] = False
    hard["mask"][1, [3, 77]] = True                        # problem 1: the mask leaves two points
    s, R, t, num, inl, success, counts, sums, best, rounds = _ransac(hard, 3)
    assert success.tolist() == [False, False, True] and best[0] == -1 and best[1] == -1
    for b in (0, 1):
        assert s[b] == 1 and (R[b] == np.eye(3)).all() and (t[b] == 0).all() and num[b] == 0 and not inl[b].any()
        assert (counts[b] == -1).all() and rounds[b] == 0
    # min_inliers above what a problem reaches: reported as a failure with the identity and an empty mask
    out = _ransac(sc, 3, min_inliers=270)
    assert out[5].tolist() == [True, False, True] and out[3][1] == 0 and not out[4][1].any() and out[0][1] == 1
    # replay, run-to-run, and a workspace that held something else
    first = _ransac(sc, 3)
    L = _lib.lib()
    nbytes = int(L.vggs_sim3_workspace_bytes(3, 400, 128))
    for fill in (0, 0xFF, 0x5A):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        for x, y in zip(first, _ransac(sc, 3, workspace=ws)):
            assert x.tobytes() == y.tobytes()
    # without samples= the draw comes from the generator: same generator state, same result
    a = sim3.estimate_sim3_robust(_dev(sc["src"]), _dev(sc["tgt"]), _dev(sc["max_error"]), num_hypotheses=64,
                                  generator=np.random.default_rng(5))
    b = sim3.estimate_sim3_robust(_dev(sc["src"]), _dev(sc["tgt"]), _dev(sc["max_error"]), num_hypotheses=64,
                                  generator=np.random.default_rng(5))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and bool(a[5].all())


# --- pair errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 7, 65])
def test_pair_errors_against_the_reference_and_the_torch_namesakes(S):
    pred, gt = SC.pose_set(S, 60 + S)
    rot, trans = (x.cpu().numpy() for x in metric.pose_pair_errors(_dev(pred), _dev(gt)))
    ref_r, ref_t = SC.pair_errors(pred, gt)
    f_r, f_t = SC.pair_errors(pred, gt, np.float64)
    assert rot.shape == trans.shape == (S * (S - 1) // 2,)
    for what, g, f, r in (("rotation", rot, f_r, ref_r), ("translation", trans, f_t, ref_t)):
        dg, df = float(np.abs(g - r).max()), float(np.abs(f - r).max())
        print(f"S = {S} {what} (degrees): GPU {dg:.2e} / float64 {df:.2e} / bound {_bound(df):.2e}")
        assert dg <= _bound(df)
    # the torch namesakes on the same poses, through the 4x4 row-vector matrices camera_to_rel_deg takes.  They go
    # through unit quaternions: for errors of a degree and more both routes are accurate to a few 1e-16 / sin(angle)
    # radians, far below 1e-9 degrees
    def se3(P):
        M = torch.zeros(len(P), 4, 4, dtype=torch.float64)
        M[:, :3, :3] = torch.from_numpy(P[:, :, :3]).transpose(1, 2)
        M[:, 3, :3] = torch.from_numpy(P[:, :, 3])
        M[:, 3, 3] = 1
        return M

    class Cameras:
        def __init__(self, P):
            self.M = se3(P)

        def get_world_to_view_transform(self):
            return self

        def get_matrix(self):
            return self.M
    t_r, t_t = metric.camera_to_rel_deg(Cameras(pred), Cameras(gt), "cpu", 1)
    big = ref_r > 1.0
    assert np.abs(t_r.numpy() - rot)[big].max(initial=0) < 1e-9 and np.abs(t_t.numpy() - trans).max() < 1e-9


def test_pair_errors_of_identical_poses_and_of_equal_centres():
    _, gt = SC.pose_set(7, 71)
    rot, trans = (x.cpu().numpy() for x in metric.pose_pair_errors(_dev(gt), _dev(gt)))
    assert rot.max() < 1e-5 and trans.max() < 1e-5
    same = SC.same_centre_poses(gt)
    rot, trans = (x.cpu().numpy() for x in metric.pose_pair_errors(_dev(same), _dev(gt)))
    ref_r, ref_t = SC.pair_errors(same, gt)
    assert trans[0] == 90.0 and float(ref_t[0]) == 90.0       # the zero vector has no direction: loss 1, arccos(0)
    f_r, f_t = SC.pair_errors(same, gt, np.float64)          # (at the clamp arccos is ill-conditioned: the rule, not a constant)
    assert np.abs(trans - ref_t).max() <= _bound(float(np.abs(f_t - ref_t).max()))
    assert np.abs(rot - ref_r).max() <= _bound(float(np.abs(f_r - ref_r).max()))
    auc = metric.pose_auc(_dev(gt), _dev(gt), max_threshold=5)
    assert float(auc) == 1.0


# --- end to end -----------------------------------------------------------------------------------------------------------
def test_alignment_of_two_reconstructions_end_to_end():
    scn = make_scene(8, 400, "SIMPLE_PINHOLE", shared_camera=False, seed=3, outlier_frac=0.0, full_visibility=True)
    size = np.array([scn.image_size, scn.image_size])
    tgt = pc.Reconstruction.from_arrays(scn.points3D, scn.extrinsics, scn.intrinsics, scn.tracks, scn.mask, size)
    src = copy.deepcopy(tgt)
    rng = np.random.default_rng(9)
    truth = pc.Sim3d(2.5, pc.Rotation3d(SC.random_rotation(rng)), rng.normal(size=3) * 4)        # tgt_from_src
    src.transform(truth.inverse())
    n = src._n
    extent = np.ptp(tgt._xyz[:n], axis=0).max()
    sigma = 1e-4 * extent / truth.scale                      # noise in the source's units
    src._xyz[:n] += sigma * rng.normal(size=(n, 3))
    bad = rng.choice(n, size=int(0.3 * n), replace=False)
    src._xyz[bad] = rng.uniform(src._xyz[:n].min(0), src._xyz[:n].max(0), size=(len(bad), 3))
    np.random.seed(4)
    by_points = pc.align_reconstructions_via_points(src, tgt, max_error=5e-4 * extent, min_inlier_ratio=0.6)
    by_centres = pc.align_reconstructions_via_proj_centers(src, tgt, 1e-6 * extent)
    assert by_points is not None and by_centres is not None
    for name, got, tol in (("points", by_points, 1e-3), ("centres", by_centres, 1e-9)):
        ds = abs(got.scale - truth.scale) / truth.scale
        dR = np.abs(got.rotation.matrix() - truth.rotation.matrix()).max()
        dt = np.linalg.norm(got.translation - truth.translation) / extent
        print(f"align via {name}: ds {ds:.2e} dR {dR:.2e} dt {dt:.2e}")
        assert max(ds, dR, dt) < tol
    src.transform(by_points)
    ids = tgt.reg_image_ids()
    a = np.stack([src.images[i].cam_from_world.matrix() for i in ids])
    b = np.stack([tgt.images[i].cam_from_world.matrix() for i in ids])
    assert float(metric.pose_auc(_dev(a), _dev(b), max_threshold=5)) == 1.0
    (scale, R, t, ok), aligned = sim3.align_cameras(_dev(np.stack([copy.deepcopy(tgt).images[i].cam_from_world.matrix() for i in ids])),
                                                    _dev(b))
    assert bool(ok) and abs(float(scale) - 1) < 1e-12 and torch.allclose(aligned, _dev(b), atol=1e-9)
