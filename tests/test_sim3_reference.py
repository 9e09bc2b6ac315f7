"""The long-double yardstick of tests/sim3_cases.py checked by itself, on the CPU: exact transforms are recovered, R is a
rotation (also where the unconstrained solution is a reflection), a float64 np.linalg.svd Umeyama agrees, degenerate
sets are flagged, the ranking rule is a total order, the LO loop never loses support -- and the condition the device
comparison relies on: for the committed seeds no point of any case has a residual within 1e-9 max_error^2 of its
threshold, in any hypothesis and any LO round, so no point is left out of a mask or count comparison."""
import numpy as np
import pytest

from tests import sim3_cases as SC

LD = np.longdouble
FIT = SC.fit_cases()


def test_exact_transforms_are_recovered():
    rng = np.random.default_rng(1)
    for n, scale, estimate in ((3, 0.7, True), (4, 3.0, True), (50, 1e-3, True), (50, 1e3, True), (20, 1.0, False)):
        src = rng.normal(size=(n, 3))
        tgt, (s0, R0, t0) = SC._moved(rng, src, scale)
        s, R, t, ok = SC.umeyama(src, tgt, None, estimate)
        assert ok
        assert abs(s - s0) / s0 < 1e-14 and np.abs(R - R0).max() < 1e-14 and np.abs(t - t0).max() < 1e-14 * max(1, scale)


@pytest.mark.parametrize("name", [n for n, c in FIT.items() if c["valid"]])
def test_rotation_is_proper_and_float64_agrees(name):
    c = FIT[name]
    for b in range(len(c["src"])):
        w = None if c["weights"] is None else c["weights"][b]
        s, R, t, ok = SC.umeyama(c["src"][b], c["tgt"][b], w, c["estimate_scale"])
        assert ok and R.dtype == LD
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-16
        assert abs(np.linalg.det(R.astype(np.float64)) - 1) < 1e-12
        dev = SC.fit_deviation(SC.umeyama_f64(c["src"][b], c["tgt"][b], w, c["estimate_scale"]), (s, R, t), c["src"][b], w)
        print(f"{name}[{b}]: float64 svd against long double: ds {dev[0]:.2e} dR {dev[1]:.2e} dt {dev[2]:.2e}")
        assert max(dev) < 1e-9
        if "truth" in c and c["noise"] == 0.0:
            assert max(SC.fit_deviation(c["truth"][b], (s, R, t), c["src"][b], w)) < 1e-13


def test_reflection_case_is_one():
    c = FIT["reflection"]
    ds, dt = c["src"][0] - c["src"][0].mean(0), c["tgt"][0] - c["tgt"][0].mean(0)
    U, _, Vt = np.linalg.svd(dt.T @ ds)
    assert np.linalg.det(U @ Vt) < 0                      # the orthogonal Procrustes solution is a reflection
    s, R, t, ok = SC.umeyama(c["src"][0], c["tgt"][0])
    assert ok and np.linalg.det(R.astype(np.float64)) > 0.999


@pytest.mark.parametrize("name", [n for n, c in FIT.items() if not c["valid"]])
def test_degenerate_sets_are_flagged(name):
    c = FIT[name]
    w = None if c["weights"] is None else c["weights"][0]
    s, R, t, ok = SC.umeyama(c["src"][0], c["tgt"][0], w)
    assert not ok and s == 1 and np.array_equal(R, np.eye(3)) and not t.any()


def test_planar_set_is_valid_and_masked_points_do_not_matter():
    c = FIT["planar"]
    assert SC.umeyama(c["src"][0], c["tgt"][0])[3]
    c = FIT["b3_masks"]
    w = c["weights"][0]
    src = c["src"][0].copy()
    src[w == 0] = np.nan
    a, b = SC.umeyama(c["src"][0], c["tgt"][0], w), SC.umeyama(src, c["tgt"][0], w)
    assert b[3] and a[0] == b[0] and np.array_equal(a[1], b[1])


def test_ranking_rule():
    counts, sums = np.array([-1, 5, 7, 7, 7, -1]), np.array([0.0, 1.0, 3.0, 2.0, 2.0, 0.0])
    assert SC.rank_best(counts, sums) == 3
    assert SC.rank_best(np.array([-1, -1]), np.zeros(2)) == -1
    assert SC.rank_best(np.array([0, 0]), np.zeros(2)) == 0


def _hypothesis_scores(sc, b, mask=None):
    out = []
    for idx in sc["samples"][b]:
        s, R, t, ok = SC.sample_transform(sc["src"][b], sc["tgt"][b], mask, idx)
        out.append((ok, SC.score((s, R, t), sc["src"][b], sc["tgt"][b], mask, sc["max_error"][b]) if ok else None))
    return out


@pytest.mark.parametrize("H", [1, SC.SCORE_TILE - 1, SC.SCORE_TILE, SC.SCORE_TILE + 1])
def test_no_point_of_the_score_cases_is_near_its_threshold(H):
    sc = SC.score_case(H)
    assert sc["outlier"].sum(1).tolist() == [90, 90] and sc["max_error"][0] != sc["max_error"][1]
    near = invalid = 0
    for b in range(2):
        for ok, res in _hypothesis_scores(sc, b):
            invalid += not ok
            if ok:
                near += int(SC.near_threshold(res[3], None, sc["max_error"][b]).sum())
    assert near == 0 and invalid == 2 * len(range(6, H, 7))


def test_lo_loop_on_the_ransac_case_and_no_point_near_its_threshold():
    sc = SC.ransac_case()
    near = 0
    for b in range(3):
        mask = sc["mask"][b]
        scores = _hypothesis_scores(sc, b, mask)
        counts = np.array([res[0] if ok else -1 for ok, res in scores])
        sums = np.array([res[1] if ok else 0 for ok, res in scores], LD)
        assert (counts < 0).any() and (counts >= 0).sum() > 64 and (b != 2 or counts.max() < 200)
        for ok, res in scores:
            if ok:
                near += int(SC.near_threshold(res[3], mask, sc["max_error"][b]).sum())
        best = SC.rank_best(counts, sums)
        T0 = SC.sample_transform(sc["src"][b], sc["tgt"][b], mask, sc["samples"][b][best])[:3]
        T, count, rsum, inl, accepted, history = SC.local_optimisation(T0, sc["src"][b], sc["tgt"][b], mask, sc["max_error"][b], 3)
        print(f"problem {b}: winner {best} with {counts[best]} inliers; after LO {count} in {accepted} accepted rounds "
              f"({len(history) - 1} scored); true inliers {int((~sc['outlier'][b] & mask).sum())}")
        for m, r in history:
            near += int(SC.near_threshold(r, mask, sc["max_error"][b]).sum())
        assert count >= counts[best] and accepted >= (2 if b == 2 else 1) and count == inl.sum() and not inl[~mask].any()
        good = ~sc["outlier"][b] & mask
        assert (inl & good).sum() >= 0.95 * good.sum()
        for err, bound in SC.recovery(T, sc["truth"][b], sc["src"][b], inl, sc["sigma"]):
            assert err <= bound
    assert near == 0                                      # (the cap would be 1 % of a problem's points: nothing is left out)


def test_pair_errors_reference():
    pred, gt = SC.pose_set(7, 51)
    rot, trans = SC.pair_errors(pred, gt)
    assert rot.shape == trans.shape == (21,) and rot.dtype == LD
    r64, t64 = SC.pair_errors(pred, gt, np.float64)
    assert np.abs(r64 - rot).max() < 1e-10 and np.abs(t64 - trans).max() < 1e-10
    same_r, same_t = SC.pair_errors(gt, gt)
    assert same_r.max() < 1e-5 and same_t.max() < 1e-5
    # a rotation of the whole predicted set about one axis by 10 degrees changes no relative rotation error ...
    a = np.deg2rad(10.0)
    G = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    moved = np.concatenate([gt[:, :, :3] @ G.T, gt[:, :, 3:]], axis=2)
    assert SC.pair_errors(moved, gt)[0].max() < 1e-5
    # ... and a known relative rotation is measured: camera 1 of two turned by 10 degrees
    two = gt[:2].copy()
    two[1, :, :3] = G @ two[1, :, :3]
    assert abs(SC.pair_errors(two, gt[:2])[0][0] - 10.0) < 1e-9
    # equal camera centres: the relative translation is zero, its "direction" the zero vector: 90 degrees
    same_centre = SC.same_centre_poses(gt)
    assert abs(SC.pair_errors(same_centre, gt)[1][0] - 90.0) < 1e-6
