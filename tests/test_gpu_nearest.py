"""The nearest-neighbour kernels (csrc/nn/nn.hip) against the all-pairs NumPy restatement of tests/nearest_cases.py, BIT FOR
BIT: index, face, count, dist2 and closest; the same bits from a second call, from a call after calls on other data, from
either visiting order and from a grid whose in-cell order was permuted; the statistics with exact counts, sums within the
bound that holds for every order of summation and the same bits twice; radius outlier removal against the restatement."""
import math

import numpy as np
import pytest
import torch

from tests import nearest_cases as C

pytestmark = pytest.mark.gpu


def D(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _given_order(queries):
    """in place of a grid's _visit: the lanes take the queries in the given order (the A/B of DESIGN.md section 34)"""
    return torch.arange(queries.shape[0], dtype=torch.int32, device=queries.device)


def _point_grid(c):
    from vggsfm_amd import nearest
    return nearest.PointGrid(D(c["points"]), c["cell"], c["origin"], c["dims"])


def _point_outputs(out):
    return out.index.cpu().numpy(), out.dist2.cpu().numpy(), out.count.cpu().numpy(), out.distance.cpu().numpy()


def _check_points(name, got, ref):
    index, dist2, count, distance = got
    assert _bits(index, ref["index"]), (name, np.nonzero(index != ref["index"])[0][:5])
    assert _bits(count, ref["count"]), (name, np.nonzero(count != ref["count"])[0][:5])
    assert _bits(dist2, ref["dist2"]), name
    assert _bits(distance, np.sqrt(ref["dist2"])), name


@pytest.mark.parametrize("name", list(C.point_cases()))
def test_nearest_point_matches_restatement(name):
    c, ref = C.point_cases()[name], C.point_reference(name)
    grid = _point_grid(c)
    origin, dims = C.box_of(c)
    assert grid.origin == [float(o) for o in origin] and grid.dims == [int(d) for d in dims]
    cells = C.cell_ids(c["points"], origin, c["cell"], dims)
    assert _bits(grid.cells(D(c["points"])).cpu().numpy(), cells)
    order = np.argsort(cells, kind="stable").astype(np.int32)              # inside a cell: ascending original index
    assert _bits(grid.order.cpu().numpy(), order)
    assert _bits(grid.points_sorted.cpu().numpy(), c["points"][order])
    start = np.searchsorted(cells[order], np.arange(dims[0] * dims[1] * dims[2] + 1), side="left").astype(np.int32)
    assert _bits(grid.cell_start.cpu().numpy(), start)
    q = D(c["queries"])
    first = _point_outputs(grid.nearest(q, c["max_dist"], c["exclude_self"]))
    _check_points(name, first, ref)
    grid._visit = _given_order                                              # the queries as they come: no bit may change
    given = _point_outputs(grid.nearest(q, c["max_dist"], c["exclude_self"]))
    assert all(_bits(a, b) for a, b in zip(first, given)), name


def test_same_bits_twice_after_other_data_and_with_permuted_cells():
    from vggsfm_amd import nearest

    c, ref = C.point_cases()["main_r10"], C.point_reference("main_r10")
    grid, q = _point_grid(c), D(c["queries"])
    first = _point_outputs(grid.nearest(q, c["max_dist"]))
    other = C.point_cases()["outside"]
    _check_points("outside", _point_outputs(_point_grid(other).nearest(D(other["queries"]), other["max_dist"])),
                  C.point_reference("outside"))
    t = C.triangle_cases()["plane"]
    nearest.nearest_faces((D(t["vertices"]), D(t["faces"])), D(t["queries"]), t["max_dist"], t["cell"])
    again = _point_outputs(grid.nearest(q, c["max_dist"]))
    assert all(_bits(a, b) for a, b in zip(first, again))
    _check_points("main_r10", again, ref)
    # the points of every cell in another order (on the host): the rule names no order, so no bit may change
    g = np.random.default_rng(5)
    start, order = grid.cell_start.cpu().numpy(), grid.order.cpu().numpy().copy()
    pts = grid.points_sorted.cpu().numpy().copy()
    for s, e in zip(start[:-1], start[1:]):
        p = s + g.permutation(e - s)
        order[s:e], pts[s:e] = order[p], pts[p]
    assert not np.array_equal(order, grid.order.cpu().numpy())
    grid.order, grid.points_sorted = D(order), D(pts)
    permuted = _point_outputs(grid.nearest(q, c["max_dist"]))
    assert all(_bits(a, b) for a, b in zip(first, permuted))


def _face_outputs(out):
    return out.face.cpu().numpy(), out.dist2.cpu().numpy(), None if out.closest is None else out.closest.cpu().numpy()


@pytest.mark.parametrize("name", list(C.triangle_cases()))
def test_nearest_face_matches_restatement(name):
    from vggsfm_amd import nearest

    c, ref = C.triangle_cases()[name], C.triangle_reference(name)
    grid = nearest.TriangleGrid(D(c["vertices"]), D(c["faces"]), c["cell"], c["origin"], c["dims"])
    origin, dims = C.box_of(c)
    assert grid.origin == [float(o) for o in origin] and grid.dims == [int(d) for d in dims]
    # the pair list: face by face, the cells of a face in row-major order, then a stable sort by cell
    lo, hi = C.face_boxes(ref["triangles"], origin, c["cell"], dims)
    cells, owners = [], []
    for f in np.nonzero(ref["valid"])[0]:
        c2, c1, c0 = np.meshgrid(*(np.arange(lo[f, a], hi[f, a] + 1) for a in (2, 1, 0)), indexing="ij")
        ids = ((c2 * dims[1] + c1) * dims[0] + c0).reshape(-1)
        cells.append(ids)
        owners.append(np.full(len(ids), f))
    cells = np.concatenate(cells) if cells else np.zeros(0, np.int64)
    owners = np.concatenate(owners) if owners else np.zeros(0, np.int64)
    perm = np.argsort(cells, kind="stable")
    assert grid.num_pairs == len(cells)
    assert _bits(grid.cell_faces.cpu().numpy(), owners[perm].astype(np.int32))
    assert _bits(grid.cell_start.cpu().numpy(),
                 np.searchsorted(cells[perm], np.arange(dims[0] * dims[1] * dims[2] + 1), side="left").astype(np.int32))
    q = D(c["queries"])
    face, dist2, closest = _face_outputs(grid.nearest(q, c["max_dist"], return_closest=True))
    assert _bits(face, ref["face"]), (name, np.nonzero(face != ref["face"])[0][:5])
    assert _bits(dist2, ref["dist2"]), name
    assert np.array_equal(np.isnan(closest), np.isnan(ref["closest"])) and _bits(np.nan_to_num(closest), np.nan_to_num(ref["closest"])), name
    assert np.isnan(closest[face < 0]).all() and np.isinf(dist2[face < 0]).all()
    for given in (False, True):                                             # closest off; the visiting order changes no bit
        if given:
            grid._visit = _given_order
        f2, d2, none = _face_outputs(grid.nearest(q, c["max_dist"]))
        assert none is None and _bits(f2, face) and _bits(d2, dist2), (name, given)


def test_distance_stats_are_exact_in_counts_bounded_in_sums_and_reproducible():
    from vggsfm_amd import nearest

    g = np.random.default_rng(9)
    for m in (0, 1, 63, 64, 65, 256 * 64 - 1, 256 * 64, 256 * 64 + 1, 70001):
        d2 = g.uniform(0.0, 4.0, m) ** 2
        d2[g.uniform(size=m) < 0.2] = np.inf
        taus = [0.5, 1.0, 1.0000001, 3.9, 4.5, 0.0, 2.0, 1e-3][:m % 9 if m < 9 else 8]
        found, below, sum_d, sum_d2 = C.distance_stats(d2, taus)
        a, b = nearest.distance_stats(D(d2), taus), nearest.distance_stats(D(d2), taus)
        assert a == b and (a.num, a.found, a.below) == (m, found, below), m
        # |computed - exact| <= (n - 1) u sum|x| / (1 - (n - 1) u) for ANY order of n additions; M 2^-53 sum|x| states it
        # (the correctly rounded sqrt adds at most 2^-53 per term, inside the same bound taken with M in place of M - 1)
        print(f"M = {m}: sum_d off by {abs(a.sum_d - sum_d):.3e} (bound {m * 2.0 ** -53 * sum_d:.3e}), "
              f"sum_d2 off by {abs(a.sum_d2 - sum_d2):.3e} (bound {m * 2.0 ** -53 * sum_d2:.3e})")
        assert abs(a.sum_d - sum_d) <= m * 2.0 ** -53 * sum_d and abs(a.sum_d2 - sum_d2) <= m * 2.0 ** -53 * sum_d2, m
    ref = C.point_reference("main_r10")
    s = nearest.distance_stats(D(ref["dist2"]), [0.1, 0.2])
    assert (s.found, s.below) == C.distance_stats(ref["dist2"], [0.1, 0.2])[:2]
    with pytest.raises(ValueError, match="at most 8"):
        nearest.distance_stats(D(d2), [0.1] * 9)


def test_radius_outlier_removal_matches_restatement():
    from vggsfm_amd import fusion, nearest

    c = C.point_cases()["nonfinite"]
    pts, radius, need = c["points"], 0.35 * C.CELL, 3
    want = C.radius_outlier_mask(pts, radius, need)
    keep = nearest.filter_radius_outliers(D(pts), radius, need)
    assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), want) and 0.1 < want.mean() < 0.95
    assert not want[[0, 17, 300]].any()                                     # a non-finite point has no neighbours
    n = len(pts)
    cloud = fusion.FusedCloud(D(pts), D(np.zeros((n, 3), np.float32)), None, D(np.arange(n, dtype=np.int32)),
                              D(np.zeros(n, np.int32)), D(np.zeros((n, 2), np.int32)))
    keep2, kept = nearest.filter_radius_outliers(cloud, radius, need)
    assert torch.equal(keep2, keep) and kept.rgb is None and _bits(kept.xyz.cpu().numpy(), pts[want])
    assert np.array_equal(kept.num_views.cpu().numpy(), np.nonzero(want)[0].astype(np.int32))
