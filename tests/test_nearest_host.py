"""CPU tests of the nearest-neighbour library: what its C-ABI registry has of its own (the registry itself is
tests/test_side_libraries.py's), what the entries refuse, the yardstick of the GPU tests (the all-pairs NumPy restatement of
tests/nearest_cases.py) against independent answers -- scipy's k-d tree, a dense minimisation over barycentric samples, the
sphere's derived interval --, the kernel's candidate cells against the pairs the restatement accepts, the margins of every
decision the GPU tests compare exactly, and the metric formulas on a hand-computed example.  No kernel is called here."""
import math
import os
import re

import numpy as np
import pytest

from tests import nearest_cases as C
from tests.test_c_abi import _parse_header
from vggsfm_amd import _lib_nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vggn_build_arch", "vggn_point_cells", "vggn_gather_points", "vggn_cell_start", "vggn_nearest_point",
         "vggn_face_cell_counts", "vggn_face_cell_pairs", "vggn_nearest_face", "vggn_distance_stats"]
GAP_FLOOR = 1e-12          # relative to r2; rounding differences would show at 1e-16


# --------------------------------------------------------------------------------------------------- registry
def test_header_table_and_library_agree():
    """What only the search has (tests/test_side_libraries.py compares table, header and symbols): the names and prototypes
    pinned by hand, and the header's constants against the binding and the restatement."""
    header = open(_lib_nn.HEADER_PATH).read()
    functions, _ = _parse_header(header)
    assert list(_lib_nn.SIGNATURES) == list(functions) == NAMES
    grid = ["double"] * 4 + ["int"] * 3
    assert functions["vggn_build_arch"] == ("pointer", [])
    assert functions["vggn_point_cells"] == ("int", ["pointer", "int"] + grid + ["pointer", "pointer"])
    assert functions["vggn_nearest_point"][1] == ["pointer"] * 3 + ["int"] + grid + ["pointer", "pointer", "int", "double", "double",
                                                                                      "int"] + ["pointer"] * 4
    assert functions["vggn_face_cell_pairs"][1] == ["pointer", "int", "pointer", "int"] + grid + ["pointer", "long"] + ["pointer"] * 3
    assert functions["vggn_nearest_face"][1] == ["pointer", "int", "pointer", "int", "pointer", "pointer", "int"] + grid + \
        ["pointer", "pointer", "int", "double", "double"] + ["pointer"] * 4
    assert functions["vggn_distance_stats"][1] == ["pointer", "int", "pointer", "int"] + ["pointer"] * 4
    consts = {k: int(v) for k, v in re.findall(r"#define VGGN_(\w+) (\d+)", header)}
    assert consts == dict(MAX_CELLS=_lib_nn.MAX_CELLS, MAX_THRESHOLDS=_lib_nn.MAX_THRESHOLDS, STATS_GROUPS=_lib_nn.STATS_GROUPS,
                          STATS_WORDS=_lib_nn.STATS_WORDS)
    assert consts["MAX_CELLS"] == 2 ** 25 and consts["MAX_THRESHOLDS"] == 8 and consts["STATS_GROUPS"] == C.STATS_GROUPS


def test_the_dense_metrics_sum_on_the_device():
    """No torch.sum below the docstring of utils/dense_metric.py: the counts and sums are vggn_distance_stats'."""
    text = open(os.path.join(ROOT, "vggsfm_amd", "utils", "dense_metric.py")).read()
    assert "torch.sum" not in text.split('"""', 2)[2]


# --------------------------------------------------------------------------------------------------- refusals
def test_host_refusals_need_no_device():
    """What the entries refuse is decided on the host, before any launch (NULL pointers throughout): every out-of-range
    argument returns VGG_ERR_INVALID_ARGUMENT even where nothing would be done, the no-ops return VGG_OK, and Python refuses
    the same arguments first."""
    import ctypes

    L = _lib_nn.lib()
    nan, inf = float("nan"), float("inf")
    good = dict(n=5, m=4, V=6, F=3, P=7, cell=0.5, dims=(5, 3, 2), r=0.4, r2=0.16, K=2)
    taus = (ctypes.c_double * 8)(*([0.1] * 8))

    def grid(a):
        return (0.0, 0.0, 0.0, a["cell"], *a["dims"])

    def cells(**kw):
        a = dict(good, **kw)
        return L.vggn_point_cells(None, a["n"], *grid(a), None, None)

    def nearest(**kw):
        a = dict(good, **kw)
        return L.vggn_nearest_point(None, None, None, a["n"], *grid(a), None, None, a["m"], a["r"], a["r2"], 0, None, None, None, None)

    def counts(**kw):
        a = dict(good, **kw)
        return L.vggn_face_cell_counts(None, a["V"], None, a["F"], *grid(a), None, None)

    def pairs(**kw):
        a = dict(good, **kw)
        return L.vggn_face_cell_pairs(None, a["V"], None, a["F"], *grid(a), None, a["P"], None, None, None)

    def faces(**kw):
        a = dict(good, **kw)
        return L.vggn_nearest_face(None, a["V"], None, a["F"], None, None, a["P"], *grid(a), None, None, a["m"], a["r"], a["r2"],
                                   None, None, None, None)

    def stats(**kw):
        a = dict(good, **kw)
        return L.vggn_distance_stats(None, a["m"], taus, a["K"], None, None, None, None)
    bad_grid = (dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(dims=(0, 3, 2)), dict(dims=(5, -1, 2)), dict(dims=(5, 3, 0)),
                dict(dims=(2 ** 13, 2 ** 12, 2)), dict(dims=(2 ** 25 + 1, 1, 1)), dict(dims=(2 ** 20, 2 ** 20, 2 ** 20)))
    bad_r = (dict(r=0.0), dict(r=-1.0), dict(r=nan), dict(r2=nan), dict(r2=-1.0))
    for entry, refused, noop in (
            (cells, bad_grid + (dict(n=-1),), dict(n=0)),
            (nearest, bad_grid + bad_r + (dict(n=-1), dict(m=-1)), dict(m=0)),
            (counts, bad_grid + (dict(V=-1), dict(F=-1)), dict(F=0)),
            (pairs, bad_grid + (dict(V=-1), dict(F=-1), dict(P=-1), dict(P=2 ** 31)), dict(F=0)),
            (faces, bad_grid + bad_r + (dict(V=-1), dict(F=-1), dict(P=-1), dict(m=-1)), dict(m=0))):
        assert entry() == -1, entry.__name__                                      # NULL pointers with work to do
        assert entry(**noop) == 0, entry.__name__
        for bad in refused:
            assert entry(**dict(noop, **bad)) == -1, (entry.__name__, bad)        # refused even where nothing would be done
    assert cells(dims=(2 ** 13, 2 ** 12, 1), n=0) == 0 and pairs(P=0) == 0 and pairs(P=2 ** 31 - 1, F=0) == 0
    # N = 0, F = 0: the queries still get "none", so the outputs are needed
    assert nearest(n=0) == -1 and faces(F=0) == -1 and faces(P=0) == -1
    for bad in (dict(m=-1), dict(K=-1), dict(K=9)):
        assert stats(**bad) == -1, bad
    assert stats() == -1 and stats(m=0) == -1                                     # (the zeros are still written: NULL outputs)
    assert L.vggn_distance_stats(None, 0, None, 1, None, None, None, None) == -1  # thresholds missing
    assert L.vggn_gather_points(None, None, -1, None, None) == -1 and L.vggn_gather_points(None, None, 0, None, None) == 0
    assert L.vggn_gather_points(None, None, 3, None, None) == -1
    for bad in ((-1, 4), (3, 0), (3, 2 ** 25 + 1)):
        assert L.vggn_cell_start(None, *bad, None, None) == -1, bad
    assert L.vggn_cell_start(None, 0, 4, None, None) == -1

    import torch
    from vggsfm_amd import nearest
    p = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        nearest.PointGrid(p, 0.5)
    with pytest.raises(ValueError, match=r"must be \(N,3\)"):
        nearest.PointGrid(torch.zeros(4, 2), 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        nearest.distance_stats(torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="dist2 must be"):
        nearest.distance_stats(torch.zeros(4, dtype=torch.float32))
    for bad in (0.0, -1.0, nan):
        with pytest.raises(ValueError, match="max_dist must be > 0"):
            nearest._radius(bad)
        with pytest.raises(ValueError, match="cell must be > 0"):
            nearest._box(p, bad, None, None)
    with pytest.raises(ValueError, match="every dim must be >= 1"):
        nearest._box(p, 0.5, [0.0, 0.0, 0.0], [3, 0, 2])
    with pytest.raises(ValueError, match="more than 2\\^25 cells: choose a larger cell"):
        nearest._box(p, 0.5, [0.0, 0.0, 0.0], [2 ** 13, 2 ** 12, 2])
    with pytest.raises(ValueError, match="given together"):
        nearest._box(p, 0.5, [0.0, 0.0, 0.0], None)
    assert nearest._box(torch.tensor([[0.0, 1.0, 2.0], [1.0, 1.0, nan], [0.9, 1.6, 2.0]], dtype=torch.float64), 0.5, None, None) == \
        (0.5, [0.0, 1.0, 2.0], [2, 2, 1])
    assert nearest._radius(0.3) == (0.3, 0.3 * 0.3) and inf > 0


# --------------------------------------------------------------------------------- the restatement against truth
@pytest.mark.parametrize("name", [n for n, c in C.point_cases().items() if len(c["points"]) and len(c["queries"])])
def test_point_restatement_matches_the_kd_tree(name):
    """scipy's k-d tree (another structure, another arithmetic): the two nearest within max_dist.  The indices are equal
    wherever the tree's two nearest distances differ, the distance is equal to 1 ulp, and the counts are the tree's ball
    counts wherever no candidate lies within 1e-9 of the radius."""
    from scipy.spatial import cKDTree

    c, ref = C.point_cases()[name], C.point_reference(name)
    keep = np.isfinite(c["points"]).all(1)
    rows = np.nonzero(keep)[0]
    tree = cKDTree(c["points"][keep])
    fq = np.isfinite(c["queries"]).all(1)
    assert (ref["index"][~fq] == -1).all() and np.isinf(ref["dist2"][~fq]).all() and (ref["count"][~fq] == 0).all()
    q = c["queries"][fq]
    k = 3 if c["exclude_self"] else 2
    d, i = tree.query(q, k=min(k, len(rows)), distance_upper_bound=c["max_dist"] * (1 + 1e-9))
    d, i = d.reshape(len(q), -1), i.reshape(len(q), -1)
    if c["exclude_self"]:                                            # drop the query's own row from its candidates
        own = rows[np.minimum(i, len(rows) - 1)] == np.nonzero(fq)[0][:, None]
        assert (own[:, 0] | (d[:, 0] > 0)).all()
        d = np.where(own, np.inf, d)
        order = np.argsort(d, axis=1, kind="stable")
        d, i = np.take_along_axis(d, order, 1), np.take_along_axis(i, order, 1)
    found = np.isfinite(d[:, 0]) & (d[:, 0] <= c["max_dist"])
    mine = ref["index"][fq]
    near_r = np.abs(d[:, 0] - c["max_dist"]) < 1e-9
    assert np.array_equal(mine[~near_r] >= 0, found[~near_r])
    both = found & (mine >= 0)
    dist = np.sqrt(ref["dist2"][fq])
    assert (np.abs(dist[both] - d[both, 0]) <= np.spacing(d[both, 0])).all()
    distinct = both & ((d.shape[1] < 2) | (d[:, min(1, d.shape[1] - 1)] != d[:, 0]))
    assert np.array_equal(mine[distinct], rows[i[distinct, 0]])
    assert distinct.sum() >= (0.95 if not c["tie"] else 0.5) * both.sum()
    ball = tree.query_ball_point(q, c["max_dist"], return_length=True) - (1 if c["exclude_self"] else 0)
    calm = ref["gap_r2"] > 1e-9
    assert not calm or np.array_equal(ball, ref["count"][fq]), name


def test_ties_go_to_the_lowest_index():
    c, ref = C.point_cases()["ties"], C.point_reference("ties")
    assert ref["index"][:5].tolist() == [3, 7, 3, 7, 5] and ref["dist2"][:4].tolist() == [0.0] * 4
    assert ref["dist2"][4] == 0.25 * 0.25 and ref["gap_best"] == 0.0                  # the midpoint: both at exactly 1/4
    assert ref["count"][0] == ref["count"][2] >= 3                                    # the three copies are all counted


@pytest.mark.parametrize("name", list(C.triangle_cases()))
def test_triangle_restatement_matches_dense_sampling(name):
    """Every valid triangle sampled on a barycentric lattice: the smallest sampled distance is an upper bound of the true one
    and within (longest edge) / n of it."""
    c, ref = C.triangle_cases()[name], C.triangle_reference(name)
    tri = ref["triangles"][ref["valid"]]
    fq = np.isfinite(c["queries"]).all(1)
    assert (ref["face"][~fq] == -1).all() and np.isnan(ref["closest"][~fq]).all()
    if not len(tri):
        assert (ref["face"] == -1).all() and np.isinf(ref["dist2"]).all() and np.isnan(ref["closest"]).all()
        return
    q = c["queries"][fq][:150]
    sampled, slack = C.sampled_distance(tri, q, 96 if name == "large_face" else 32)
    d = np.sqrt(ref["dist2"][fq][:150])
    found = np.isfinite(d)
    assert found.sum() >= 5, name
    assert (d[found] <= sampled[found] + 1e-12).all() and (sampled[found] - d[found] <= slack).all()
    assert (sampled[~found] > c["max_dist"] - 1e-12).all()
    # the closest point is at that distance, and it lies on the winner's plane
    x, f = ref["closest"][fq][:150][found], ref["face"][fq][:150][found]
    assert np.abs(np.linalg.norm(q[found] - x, axis=1) - d[found]).max() < 1e-14
    t = ref["triangles"][f]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    assert np.abs(((x - t[:, 0]) * n).sum(1) / np.linalg.norm(n, axis=1)).max() < 1e-13
    assert ref["valid"][f].all()


def test_sphere_distance_lies_in_the_derived_interval():
    """Vertices on the sphere of radius R, longest edge L: the mesh lies between the sphere and the sphere of radius
    R - sag, sag = R - sqrt(R^2 - L^2 / 3) (the circumradius of a face is at most L / sqrt 3).  So for a point at radius
    rho > R the distance lies in [rho - R, rho - R + sag] -- up to the angular gap to the nearest mesh point, bounded by the
    same sag along the radius."""
    c, ref = C.triangle_cases()["sphere"], C.triangle_reference("sphere")
    R = C.SPHERE_R
    assert len(c["faces"]) == 512 and np.abs(np.linalg.norm(c["vertices"], axis=1) - R).max() < 1e-15
    tri = ref["triangles"]
    L = np.linalg.norm(tri - np.roll(tri, 1, axis=1), axis=-1).max()
    sag = R - math.sqrt(R * R - L * L / 3.0)
    rho = np.linalg.norm(c["queries"], axis=1)
    out = rho > R
    d = np.sqrt(ref["dist2"])
    assert out.sum() > 100 and np.isfinite(d[out]).all()
    print(f"\nsphere: longest edge {L:.4f}, sag {sag:.5f}; d - (rho - R) in [{(d - rho + R)[out].min():.2e}, {(d - rho + R)[out].max():.2e}]")
    assert ((d - (rho - R))[out] >= -1e-14).all() and ((d - (rho - R))[out] <= sag + 1e-14).all()
    inside = rho < R - sag
    assert inside.sum() > 50 and ((R - rho)[inside] - d[inside] <= sag + 1e-14).all() and (d[inside] <= (R - rho)[inside] + 1e-14).all()


def test_queries_fall_in_each_of_the_seven_regions():
    _, labels = C.region_queries()
    ref = C.triangle_reference("regions")
    assert [C.REGIONS[r] for r in ref["region"]] == labels and set(labels) == set(C.REGIONS)
    # and the other cases meet every region too
    seen = set()
    for name in ("plane", "sphere", "large_face"):
        seen |= set(C.triangle_reference(name)["region"].tolist())
    assert seen >= set(range(7))
    sk = C.triangle_reference("skippable")
    assert sk["valid"].tolist() == [False] * 8 + [True, False, False] and set(np.unique(sk["face"])) == {-1, 8}


# --------------------------------------------------------------------------------------------- margins and ties
def test_every_accepted_pair_lies_in_the_kernels_candidate_cells():
    """The restatement has no grid; the kernel's range of cells is the header's.  For every case: the cell of the point of
    every accepted (query, point) pair lies inside the query's range, and every accepted (query, face) pair has a cell of
    the face's box inside the query's range.  The main grid holds the occupancies the kernel's loops can get wrong."""
    for name, c in C.point_cases().items():
        origin, dims = C.box_of(c)
        qi, pi = C.point_reference(name)["accepted"]
        lo, hi = C.query_range(c["queries"], c["max_dist"], origin, c["cell"], dims)
        pc = C.axis_cells(c["points"][pi], origin, c["cell"], dims)
        assert ((pc >= lo[qi]) & (pc <= hi[qi])).all(), name
        ids = C.cell_ids(c["points"], origin, c["cell"], dims)
        assert ids.max(initial=-1) < dims[0] * dims[1] * dims[2] and (ids >= 0).sum() == np.isfinite(c["points"]).all(1).sum()
        if name == "main_r10":
            occupancy = np.bincount(ids, minlength=30)
            assert occupancy.tolist() == [C.CELL_COUNTS[i % 6] for i in range(30)] and len(ids) == 4465
            spans = (hi - lo + 1).max(0)
            assert spans.tolist() == [5, 3, 2]
        if name == "outside":
            t = np.floor((c["points"] - np.asarray(origin)) / c["cell"])
            assert ((t < 0) | (t >= np.asarray(dims))).any(1).mean() > 0.5             # most points lie outside the box
    reach = {n: int((np.floor((c["queries"] + c["max_dist"] - C.ORIGIN) / C.CELL) - np.floor((c["queries"] - c["max_dist"] - C.ORIGIN) / C.CELL)).max() + 1)
             for n, c in C.point_cases().items() if n.startswith("main_")}
    assert reach == {"main_r04": 2, "main_r10": 3, "main_r23": 6}, reach               # cells per axis before the margin
    for name, c in C.triangle_cases().items():
        origin, dims = C.box_of(c)
        ref = C.triangle_reference(name)
        qi, fi = ref["accepted"]
        lo, hi = C.query_range(c["queries"], c["max_dist"], origin, c["cell"], dims)
        flo, fhi = C.face_boxes(ref["triangles"], origin, c["cell"], dims)
        assert ((flo[fi] <= hi[qi]) & (fhi[fi] >= lo[qi])).all(), name
        # stronger: the cell of the closest point itself lies in both
        won = ref["face"] >= 0
        xc = C.axis_cells(ref["closest"][won], origin, c["cell"], dims)
        assert ((xc >= lo[won]) & (xc <= hi[won])).all() and ((xc >= flo[ref["face"][won]]) & (xc <= fhi[ref["face"][won]])).all(), name
        if name == "large_face":
            cells = (fhi - flo + 1).prod(1)
            assert cells[0] > 3000 and cells[1:].max() < 40


def test_no_decision_of_a_gpu_case_is_a_tie():
    """The GPU tests compare bits, so outside the case that is about ties no decision may sit on its threshold: the smallest
    gap between the best and the second-best d2, and between any d2 and r2, both relative to r2, is above GAP_FLOOR.  For a
    mesh the runner-up is the best face that shares no vertex with the winner: two faces tie by construction wherever the
    closest point lies on their common edge or vertex, and there the lower index wins by the same arithmetic on both sides."""
    worst_best, worst_r2 = np.inf, np.inf
    for name, c in list(C.point_cases().items()) + list(C.triangle_cases().items()):
        ref = C.point_reference(name) if "points" in c else C.triangle_reference(name)
        print(f"{name}: best/second gap {ref['gap_best']:.3e}, d2/r2 gap {ref['gap_r2']:.3e}")
        if c["tie"]:
            continue
        assert ref["gap_best"] > GAP_FLOOR and ref["gap_r2"] > GAP_FLOOR, name
        worst_best, worst_r2 = min(worst_best, ref["gap_best"]), min(worst_r2, ref["gap_r2"])
    print(f"smallest gaps over the tie-free cases: best/second {worst_best:.3e}, d2/r2 {worst_r2:.3e} (floor {GAP_FLOOR:.0e})")
    assert [n for n, c in C.point_cases().items() if c["tie"]] == ["ties"]


def test_metric_formulas_on_a_hand_computed_example():
    """gt at x = 0, 1, 2, 3 and pred at x = 0, 1.25, 2.5, 10 on a line, max_dist 1: d_p = 0, 1/4, 1/2, none and
    d_g = 0, 1/4, 1/2, 1/2.  Every expected number below is worked out by hand and exact in binary."""
    from vggsfm_amd import nearest
    from vggsfm_amd.utils import dense_metric

    line = lambda xs: np.stack([np.asarray(xs, np.float64), np.zeros(len(xs)), np.zeros(len(xs))], -1)
    pred, gt, taus = line([0.0, 1.25, 2.5, 10.0]), line([0.0, 1.0, 2.0, 3.0]), [0.3, 0.6]
    stats = []
    for q, p in ((pred, gt), (gt, pred)):
        d2 = C.nearest_point(p, q, 1.0)["dist2"]
        found, below, sum_d, sum_d2 = C.distance_stats(d2, taus)
        stats.append(nearest.Stats(len(d2), found, below, sum_d, sum_d2))
    assert stats[0] == nearest.Stats(4, 3, [2, 3], 0.75, 0.3125) and stats[1] == nearest.Stats(4, 4, [2, 4], 1.25, 0.5625)
    m = dense_metric.metrics_from_stats(stats[0], stats[1], taus, 1.0)
    assert (m["num_pred"], m["num_gt"], m["found_pred"], m["found_gt"]) == (4, 4, 3, 4)
    assert m["accuracy"] == 0.25 and m["completeness"] == 0.3125 and m["overall"] == 0.28125
    assert m["accuracy_clamped"] == 0.4375 and m["completeness_clamped"] == 0.3125 and m["overall_clamped"] == 0.375
    assert m["accuracy_rms"] == math.sqrt(0.3125 / 3) and m["completeness_rms"] == 0.375
    assert m["precision"] == [0.5, 0.75] and m["recall"] == [0.5, 1.0] and m["fscore"] == [0.5, 2 * 0.75 / 1.75]
    empty = nearest.Stats(4, 0, [0, 0], 0.0, 0.0)
    m0 = dense_metric.metrics_from_stats(empty, empty, taus, 1.0)
    assert m0["fscore"] == [0.0, 0.0] and math.isnan(m0["accuracy"]) and m0["accuracy_clamped"] == 1.0
