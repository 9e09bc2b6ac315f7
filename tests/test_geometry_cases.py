"""CPU: the long-double restatement of tests/geometry_cases.py checked against the reference project's recorded results
(tests/golden/geom_regimes_*.npz, oracle/gen_golden_geometry_regimes.py) and against oracle/geometry.py, and every case
checked for what it was built to hit.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

from oracle import geometry as G
from tests import geometry_cases as C


def _recomputed(name):
    g = C.load(name)
    job = C.case_from_fixture(name, g)
    return g, job, C.evaluate(job)


def _share(adm):
    return float(np.mean(adm)) if np.size(adm) else 1.0


@pytest.mark.parametrize("name", C.FILTER_NAMES)
def test_filter_case(name):
    g, job, r = _recomputed(name)
    kw = {k: v for k, v in job["kw"].items() if k != "behind_value"}
    am, ad = g["adm_mask"], g["adm_detail"]
    ref = "ref_mask" in g
    diff = {}
    if ref:                                           # (the oracle builds the (S^2, P) angle tensor as the reference does)
        with np.errstate(all="ignore"):
            om, od = G.filter_all_points3D(job["pts"], job["tracks"].astype(np.float64), job["ext"], job["K"], job["extra"],
                                           return_detail=True, **kw)
        diff["oracle"] = (int((om != g["ld_mask"])[am].sum()), int((od != g["ld_detail"])[ad].sum()))
        diff["reference"] = (int((g["ref_mask"] != g["ld_mask"])[am].sum()), int((g["ref_detail"] != g["ld_detail"])[ad].sum()))
    print(f"\n{name}: S {job['ext'].shape[0]} P {len(job['pts'])} accepted {int(g['ld_mask'].sum())} inlier bits {int(r['inlier'].sum())} | "
          f"admitted masks {_share(am):.4f} details {_share(ad):.4f} | dev64 err {g['figures'][0]:.2e} cz {g['figures'][1]:.2e} "
          f"angle {g['figures'][2]:.2e} deg (delta = {C.MARGIN:g} x) | (mask, detail) bits differing on admitted: {diff}")
    # the fixture is what the recipe produces
    for k, v in (("ld_mask", r["mask"]), ("ld_detail", r["detail"]), ("adm_mask", r["adm_mask"]), ("adm_detail", r["adm_detail"])):
        assert np.array_equal(g[k], v), k
    assert ref == (name not in C.REFERENCE_CANNOT_RUN)
    # cap on what is left out; these cases are built so that nothing is
    assert _share(am) >= 1 - C.CAP and _share(ad) >= 1 - C.CAP
    assert am.all() and ad.all()
    assert all(d == (0, 0) for d in diff.values())
    assert np.array_equal(r["f64_mask"][am], g["ld_mask"][am]) and np.array_equal(r["f64_detail"][ad], g["ld_detail"][ad])
    # the case hits what it was built for
    e = job["expect"]
    S = job["ext"].shape[0]
    if "pair" in e:                                   # one inlier pair per point: the mask is its angle test, the detail its two bits
        want = np.zeros((S, len(e["above"])), bool)
        for p, (a, b) in enumerate(e["pair"]):
            want[a, p] = want[b, p] = e["above"][p]
        assert np.array_equal(g["ld_mask"], e["above"]) and np.array_equal(g["ld_detail"], want)
        clean = np.setdiff1d(np.arange(len(e["above"])), e.get("hit", []))
        assert (r["inlier"].sum(0)[clean] == 2).all()
        if "hit" in e:
            assert not g["ld_mask"][e["hit"]].any() and (r["inlier"].sum(0)[e["hit"]] <= 1).all()
    else:
        assert np.array_equal(g["ld_mask"], e["mask"])
    if "inliers" in e:
        assert (r["inlier"].sum(0) == e["inliers"]).all()
    if "inliers0" in e:
        assert np.array_equal(r["inlier"][0], e["inliers0"])
    if name == "full_search":
        assert (r["inlier"].sum(0) == 200).all() and (r["best"] < 1.5).all() and not g["ld_mask"].any()
    if name == "s1_chk0":
        assert np.array_equal(g["ld_detail"][0], e["inliers0"])
    if name == "between":                              # the unfolded angle is near 180 degrees
        assert (r["best"] < 25).all()


def test_pair_cases_cover_the_lanes_and_words():
    seen = set()
    for name in C.PAIR_NAMES:
        job = C.build(name)
        S = job["ext"].shape[0]
        for (a, b), up in zip(job["expect"]["pair"], job["expect"]["above"]):
            seen.add((S, int(a), int(b), bool(up)))
    lanes = {(a % 4, b % 4) for S, a, b, _ in seen if S >= 63}
    print(f"\n{len(seen)} (S, a, b, above) combinations; lane combinations at S >= 63: {len(lanes)}")
    assert len(lanes) == 16
    for S, a, b in ((65, 62, 63), (65, 63, 64), (129, 64, 65), (129, 63, 128), (129, 127, 128), (257, 0, 256), (257, 255, 256),
                    (2, 0, 1), (64, 0, 63), (128, 126, 127)):
        assert (S, a, b, True) in seen and (S, a, b, False) in seen, (S, a, b)
    assert {S for S, _, _, _ in seen} == {2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257}
    assert {1, 63, 64, 65} <= {P for _, P, _, _ in C.PAIR_SHAPES}
    assert {(k, f) for _, _, k, f in C.PAIR_SHAPES} >= {(0, False), (1, True), (2, False), (4, True), (0, True), (4, False)}


@pytest.mark.parametrize("name", C.PROJECT_NAMES)
def test_project_case(name):
    g, job, r = _recomputed(name)
    adm, cls = g["adm"], g["cls"]
    fin = adm & (cls == 0)
    with np.errstate(all="ignore"):
        opx, opc = G.project_3D_points(job["pts"], job["ext"], job["K"], job["extra"], return_points_cam=True)
    figs = {}
    for who, px, pc in (("reference", g["ref_px"], g["ref_pc"]), ("oracle", opx, opc)):
        ex_px, b_px = C.value_excess(px, g["ld_px"], g["figures"][0], fin)
        ex_pc, b_pc = C.value_excess(pc, g["ld_pc"], g["figures"][1], np.isfinite(g["ld_pc"]))
        special = int((px != g["ld_px"])[adm & (cls != 0)].sum())
        figs[who] = (ex_px, b_px, ex_pc, b_pc, special)
    print(f"\n{name}: classes finite / NaN / +max / -max {np.bincount(cls.ravel(), minlength=4)} admitted {_share(adm):.4f} | dev64 px "
          f"{g['figures'][0]:.2e} cam {g['figures'][1]:.2e} | (px deviation, bound, cam deviation, bound, special elements differing): {figs}")
    assert np.array_equal(g["ld_px"], r["px"]) and np.array_equal(g["cls"], r["cls"])
    assert adm.all()
    for ex_px, b_px, ex_pc, b_pc, special in figs.values():
        assert ex_px <= b_px and ex_pc <= b_pc and special == 0
    if name.startswith("project_k"):
        assert (np.bincount(cls.ravel(), minlength=4) >= 1).all()
        assert np.array_equal(np.unique(g["ld_px"][cls != 0]), [-C.DBL_MAX, 0.0, C.DBL_MAX])


@pytest.mark.parametrize("name", C.UNDISTORT_NAMES)
def test_undistort_case(name):
    g, job, r = _recomputed(name)
    adm = g["adm_elem"][..., None] & np.isfinite(g["ld_values"])
    if job["extra"] is None:
        oval, oit = G.cam_from_img(job["tracks"].astype(np.float64), job["K"]), 0
    else:
        u, v = C.normalise(job["tracks"], job["K"], np.float64)
        with np.errstate(all="ignore"):
            oval, oit = G.iterative_undistortion(job["extra"], np.stack([u, v], -1), max_iterations=job["max_iterations"])
    figs = {who: C.value_excess(val, g["ld_values"], g["figures"][0], adm) + (int(it),)
            for who, val, it in (("reference", g["ref_values"], g["ref_iters"]), ("oracle", oval, oit))}
    print(f"\n{name}: {g['ld_values'].shape[:2]} tracks, iterations {int(g['ld_iters'])}, count admitted {bool(g['adm_count'])}, elements "
          f"admitted {_share(g['adm_elem']):.4f}, swaps per step {g['swaps'][:4]} (smallest |u11| {r['u11_min']:.3g}) | dev64 values "
          f"{g['figures'][0]:.2e} stop {g['figures'][1]:.2e} swap {g['figures'][2]:.2e} | (deviation, bound, iterations): {figs}")
    assert np.array_equal(g["ld_values"], r["values"], equal_nan=True) and int(g["ld_iters"]) == r["iters"]
    assert bool(g["adm_count"]) and g["adm_elem"].all()
    for ex, bound, it in figs.values():
        assert ex <= bound and it == int(g["ld_iters"])
    for val in (g["ref_values"], oval):
        assert np.array_equal(np.isfinite(val), np.isfinite(g["ld_values"]))
    # the case hits what it was built for
    if name.startswith("count"):
        assert int(g["ld_iters"]) == int(name[5:])
    if name.startswith("maxit"):
        assert int(g["ld_iters"]) == int(name[5:]) < int(C.load("count17")["ld_iters"])
    if name == "nonfinite_undistort":
        bad = ~np.isfinite(g["ld_values"]).all(-1)
        assert int(g["ld_iters"]) == 100 and bad.sum() == 2 and bad[0, 3] and bad[1, 7]
    if name == "global_stop":                      # frames 0 and 2 alone would have stopped long before
        for s in (0, 2):
            alone = C._undistort(dict(job, tracks=job["tracks"][s:s + 1], K=job["K"][s:s + 1], extra=job["extra"][s:s + 1]), C.LD)
            assert alone["iters"] <= 4 < int(g["ld_iters"]) == 16
    if name.startswith("swap_it"):
        assert int(g["swaps"][0]) == C.SWAPS_STEP1 and r["u11_min"] > 0.5
    if name == "eps_step":
        u, v = C.normalise(job["tracks"], job["K"], np.float64)
        assert ((u == 0) & (v == 0)).any() and ((u == 0) & (v != 0)).any() and ((u != 0) & (v == 0)).any()
    if name == "undistort_stride":
        assert int(g["ld_iters"]) > 8
