"""GPU: the LO-RANSAC triangulation kernels on hard geometry and at their lane-structure edges, against the long-double
reference recorded in tests/golden/tri_regimes_*.npz (tests/triangulation_cases.py; the CPU half of the argument is
tests/test_triangulation_cases.py).  Bounds are the rules of triangulation_cases.py, built from what float64 does with the
reference's own formulas; every test prints its figures before it asserts."""
import contextlib

import numpy as np
import pytest
import torch

from tests import triangulation_cases as C
from tests.poison import equals_pattern, poisoned_allocations
from vggsfm_amd import _lib
from vggsfm_amd.utils import triangulation as T

pytestmark = pytest.mark.gpu
PATTERN = 0x7F


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


@contextlib.contextmanager
def spied():
    """Counts the calls of the two chunk entries on the bound library for the duration of the block and keeps what they report:
    the per-chunk maxima the asynchronous launches leave on the device, the thresholds the synchronous re-launch hands back."""
    L = _lib.lib()
    seen = dict(enqueue=0, relaunch=0, gmax=[], thresholds=None)
    enqueue, relaunch = L.vgg_triangulate_tracks_chunks_enqueue, L.vgg_triangulate_tracks_chunks

    def spy_enqueue(*a):
        seen["enqueue"] += 1
        seen["gmax"].append(a[16])
        return enqueue(*a)

    def spy_relaunch(*a):
        seen["relaunch"] += 1
        rc = relaunch(*a)
        seen["thresholds"] = np.array(list(a[15]))
        return rc

    L.vgg_triangulate_tracks_chunks_enqueue, L.vgg_triangulate_tracks_chunks = spy_enqueue, spy_relaunch
    try:
        yield seen
    finally:
        L.vgg_triangulate_tracks_chunks_enqueue, L.vgg_triangulate_tracks_chunks = enqueue, relaunch


def run(case, tracks=slice(None)):
    torch.manual_seed(case["seed"])           # the host RNG stream of the recorded reference run
    score = case["score"]
    return T.triangulate_tracks(D(case["ext"]), D(case["tn"][:, tracks]), max_ransac_iters=case["iters"],
                                track_vis=D(case["vis"][:, tracks]), track_score=None if score is None else D(score[:, tracks]),
                                max_tri_points_num=case["max_pts"])


@pytest.mark.parametrize("name", C.NAMES)
def test_case_against_long_double(name):
    g = C.load(name)
    case = C.case_from_fixture(name, g)
    with spied() as seen, poisoned_allocations(PATTERN):
        pts, num, msk = run(case)
        pts, num, msk = pts.cpu().numpy(), num.cpu().numpy(), msk.cpu().numpy()
        reported = seen["thresholds"] if seen["relaunch"] else \
            torch.cat(seen["gmax"]).cpu().numpy().view(np.float64) + 1e-6
    adm, ivc = g["ld_admitted"], C.invalid_vis_conf(case)
    bound = max(C.POINT_FLOOR, C.MARGIN * float(g["ld_dev64"]))
    cmp = adm & (g["ld_num"] >= 2)
    dev = C.rel_point_distance(pts, g["ld_points"], case["size"])
    thr_dev = np.abs(reported - g["ld_thresholds"]) / g["ld_thresholds"]
    worst = float(dev[cmp].max()) if cmp.any() else 0.0
    print(f"\n{name}: S {case['tn'].shape[0]} N {len(adm)} admitted {int(adm.sum())} ({1 - adm.mean():.4f} left out) | mask bits "
          f"differing on admitted {int((msk[adm] != g['ld_mask'][adm]).sum())}, on the rest {int((msk[~adm] != g['ld_mask'][~adm]).sum())} | "
          f"point deviation {worst:.3e} (bound {bound:.3e}, dev64 {float(g['ld_dev64']):.3e}) | thresholds {reported} "
          f"deviation {thr_dev.max():.2e} | enqueue {seen['enqueue']} relaunch {seen['relaunch']}")
    assert not equals_pattern(pts, PATTERN).any() and not equals_pattern(num, PATTERN).any()        # every element written
    assert np.array_equal(num, msk.sum(1)) and not (msk & ivc).any()
    assert np.array_equal(msk[adm], g["ld_mask"][adm]) and np.array_equal(num[adm], g["ld_num"][adm])
    assert worst <= bound
    # (the thresholds of the multi-chunk cases to THRESHOLD_RTOL; elsewhere the largest mean inlier error is an arc cosine
    #  that float64 itself only has to thr_dev64, and the rule is the one of the points)
    thr_dev64 = np.abs(g["ld_thresholds64"] - g["ld_thresholds"]) / g["ld_thresholds"]
    assert (thr_dev <= (C.THRESHOLD_RTOL if name in C.MULTI_CHUNK else np.maximum(C.THRESHOLD_RTOL, C.MARGIN * thr_dev64))).all()
    if name in C.RETHRESHOLD:                     # the call went through the synchronous re-launch with the measured thresholds
        assert (g["ld_thresholds"] < 2 * np.pi).all() and seen["relaunch"] >= 1


@pytest.mark.parametrize("group", C.PAIR_GROUPS)
def test_two_view_eigenvector(group):
    """vgg_triangulate_by_pair is the two-view hypothesis (0, s) of the RANSAC kernel bit for bit: the eigen-solver alone."""
    g = C.load(C.pair_name(group))
    src = g if group == "pair_sweep" else C.load(group)
    with poisoned_allocations(PATTERN):
        pts, che, ang = T.triangulate_by_pair(D(src["ext"])[None], D(src["tn"])[None])
        pts, che, ang = pts.cpu().numpy(), che.cpu().numpy(), ang.cpu().numpy()
    gap, unit = C.pair_condition(g["ld_lam"])
    big = gap >= C.GAP_MIN
    with np.errstate(all="ignore"):
        ratio = C.direction_angle(pts, g["ld_points"]) / unit
    flagged = np.isfinite(pts).all(-1) | ~che | (ang == 0)
    print(f"\n{group}: {big.size} inputs, {int(big.sum())} with a relative gap >= {C.GAP_MIN:g} (smallest {np.nanmin(gap):.2e}) | largest "
          f"angle / (eps lambda_4 / gap) {np.nanmax(ratio[big]):.3f} (bound {C.PAIR_C:g}) | below the gap: {int((~big).sum())}, "
          f"not finite-or-flagged {int((~flagged[~big]).sum())}, NaN angles {int(np.isnan(ang).sum())}")
    assert not equals_pattern(pts, PATTERN).any()
    assert not (ratio[big] > C.PAIR_C).any() and not np.isnan(ratio[big]).any()
    assert flagged[~big].all()
    assert not (np.isnan(ang) & ~np.isnan(g["ld_ang"])).any()


@pytest.mark.parametrize("name", ["arc", "dup", "viscount"])
def test_batch_independence(name):
    """One launch and the two halves of its tracks (one reference chunk each, so the same pairs): the same bits."""
    case = C.case_from_fixture(name)
    N = case["tn"].shape[1]
    whole = run(case)
    halves = [run(case, slice(0, N // 2 + 1)), run(case, slice(N // 2 + 1, N))]
    same = [torch.equal(w.view(torch.int64) if w.dtype == torch.float64 else w,
                        torch.cat([a, b]).view(torch.int64) if w.dtype == torch.float64 else torch.cat([a, b]))
            for w, a, b in zip(whole, *halves)]
    print(f"\n{name}: points / counts / masks identical: {same}")
    assert all(same)
