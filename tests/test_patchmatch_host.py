"""CPU tests of the PatchMatch refinement: what its C-ABI registry has of its own (the registry itself is
tests/test_side_libraries.py's), what the entries refuse, the hash, the yardstick of the GPU tests (the NumPy restatement of
tests/patchmatch_cases.py) against analytic truth and against the sweep it starts from, the structure of a step, and the
margins of every decision the GPU tests compare exactly.  No kernel is called here."""
import re

import numpy as np
import pytest

from tests import patchmatch_cases as P
from tests.test_c_abi import _parse_header
from vggsfm_amd import _lib_patchmatch

NAMES = ["vggr_build_arch", "vggr_plane_init", "vggr_plane_cost", "vggr_step", "vggr_outputs"]


# --------------------------------------------------------------------------------------------------- registry
def test_header_table_and_library_agree():
    """What only the refinement has (tests/test_side_libraries.py compares table, header and symbols): the names and
    prototypes pinned by hand, and the header's constants against the binding and the restatement."""
    header = open(_lib_patchmatch.HEADER_PATH).read()
    functions, _ = _parse_header(header)
    assert list(_lib_patchmatch.SIGNATURES) == list(functions) == NAMES
    assert functions["vggr_build_arch"] == ("pointer", [])
    assert functions["vggr_plane_init"][1] == ["pointer"] * 4 + ["int"] * 4 + ["double"] * 3 + ["unsigned long long", "pointer", "pointer"]
    assert functions["vggr_plane_cost"][1] == ["pointer"] * 4 + ["int"] * 4 + ["pointer", "int", "int", "int", "double"] + ["pointer"] * 3
    assert functions["vggr_step"][1] == ["pointer"] * 4 + ["int"] * 4 + ["pointer", "int", "int", "int"] + ["double"] * 6 + \
        ["unsigned long long", "int", "int"] + ["pointer"] * 3
    assert functions["vggr_outputs"][1] == ["pointer"] * 4 + ["int"] * 4 + ["double"] + ["pointer"] * 4
    consts = dict(re.findall(r"#define VGGR_(\w+) (\d+)", header))
    assert [int(consts[k]) for k in ("MAX_SOURCES", "MAX_RADIUS")] == [_lib_patchmatch.MAX_SOURCES, _lib_patchmatch.MAX_RADIUS] \
        == [P.MAX_SOURCES, P.MAX_RADIUS]                                            # (and the stereo's: test_side_libraries.py)


# --------------------------------------------------------------------------------------------------- refusals
def test_host_refusals_need_no_device():
    """What the entries refuse is decided on the host, before any launch (sources is a host array): every out-of-range
    argument returns VGG_ERR_INVALID_ARGUMENT, an empty frame is a no-op."""
    import torch
    L = _lib_patchmatch.lib()
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    nan, inf = float("nan"), float("inf")
    good = dict(num_frames=3, height=4, width=5, ref=1, sources=i32(0, 2), num_sources=2, radius=2, min_views=1, far=0.2, near=0.3,
                dstep=0.01, sstep=0.5, cos=0.26, seed=0, iteration=0, colour=0, min_conf=0.5)
    views = (dict(ref=-1), dict(ref=3), dict(num_frames=0), dict(height=-1), dict(width=-1))
    sources = (dict(radius=0), dict(radius=4), dict(num_sources=0), dict(min_views=0), dict(min_views=3), dict(sources=i32(0, 3)),
               dict(sources=i32(-1, 2)), dict(sources=i32(1, 2)), dict(sources=None),
               dict(sources=i32(*range(2, 11)), num_sources=9, num_frames=12))
    ranges = (dict(far=0.0), dict(far=-0.1), dict(far=0.3, near=0.2), dict(far=0.25, near=0.25), dict(near=inf), dict(far=nan),
              dict(near=nan), dict(cos=-0.1), dict(cos=1.5), dict(cos=nan))

    def init(**kw):
        a = dict(good, **kw)
        return L.vggr_plane_init(None, None, None, None, a["num_frames"], a["height"], a["width"], a["ref"], a["far"], a["near"],
                                 a["cos"], a["seed"], None, None)

    def cost(**kw):
        a = dict(good, **kw)
        return L.vggr_plane_cost(None, None, None, None, a["num_frames"], a["height"], a["width"], a["ref"], a["sources"],
                                 a["num_sources"], a["radius"], a["min_views"], 1e-5, None, None, None)

    def step(**kw):
        a = dict(good, **kw)
        return L.vggr_step(None, None, None, None, a["num_frames"], a["height"], a["width"], a["ref"], a["sources"], a["num_sources"],
                           a["radius"], a["min_views"], 1e-5, a["far"], a["near"], a["dstep"], a["sstep"], a["cos"], a["seed"],
                           a["iteration"], a["colour"], None, None, None)

    def outs(**kw):
        a = dict(good, **kw)
        return L.vggr_outputs(None, None, None, None, a["num_frames"], a["height"], a["width"], a["ref"], a["min_conf"], None, None,
                              None, None)
    for entry, refused in ((init, views + ranges), (cost, views + sources),
                           (step, views + sources + ranges + (dict(colour=-1), dict(colour=2), dict(iteration=-1), dict(dstep=-1e-3),
                                                              dict(dstep=nan), dict(dstep=inf), dict(sstep=-0.5), dict(sstep=nan))),
                           (outs, views + (dict(min_conf=nan),))):
        assert entry(height=0) == 0 and entry(width=0) == 0, entry.__name__      # a frame of 0 pixels: a no-op
        assert entry() == -1, entry.__name__                                      # NULL pointers with pixels to work on
        for bad in refused:
            assert entry(**dict({"height": 0} if "height" not in bad and "width" not in bad else {}, **bad)) == -1, (entry.__name__, bad)
    assert step(height=0, iteration=5000, colour=1, dstep=0.0, sstep=0.0, cos=0.0) == 0 and step(height=0, cos=1.0) == 0
    assert init(height=0, seed=2 ** 64 - 1) == 0
    with pytest.raises(Exception):
        init(height=0, seed=-1)                                                   # the binding refuses what does not fit


# --------------------------------------------------------------------------------------------------- hash
def test_hash_against_written_values():
    """The restated hash against values computed with Python integers when the test was written (mix(golden) is
    splitmix64's first output for seed 0), the exact scaling of the top 53 bits, and a vector of pixels at once."""
    assert int(P.mix(0)) == 0 and int(P.mix(1)) == 0x5692161D100B05E5 and int(P.mix(0x9E3779B97F4A7C15)) == 0xE220A8397B1DCDAF
    known = {(0, 0, 0, 0, 0): (0x552D806A62B97855, 0.3327255496721814, -0.33454890065563725),
             (0, 0, 1, 0, 0): (0x6AF8A94FC9C425F5, 0.4178567714495931, -0.1642864571008138),
             (7, 3, 1, 767, 2): (0xFEA26A1F03A76371, 0.9946657491415443, 0.9893314982830885),
             (2 ** 63 - 1, 2 ** 64 - 1, 0, 1234, 0): (0x5763967DA508F5A2, 0.34136334006783264, -0.3172733198643347),
             (1, 2, 0, 34, 1): (0x81BB8C88AF0EE5C3, 0.506768020029138, 0.013536040058276022)}
    for words, (h, u, s) in known.items():
        got = P.hash5(*words)
        assert int(got) == h and float(P.unit(got)) == u and float(P.signed(got)) == s, words
    pixels = np.array([0, 34, 767, 1234], np.uint64)
    vec = P.hash5(7, 3, 1, pixels, 2)
    assert vec.dtype == np.uint64 and [int(v) for v in vec] == [int(P.hash5(7, 3, 1, int(p), 2)) for p in pixels]
    assert int(vec[2]) == 0xFEA26A1F03A76371 and P.INIT_ITERATION == 2 ** 64 - 1
    top = np.uint64(2 ** 64 - 1)
    assert float(P.unit(top)) == 1.0 - 2.0 ** -53 and float(P.signed(top)) == 1.0 - 2.0 ** -52 and float(P.signed(0)) == -1.0
    draws = P.signed(P.hash5(0, 0, 0, np.arange(4096, dtype=np.uint64), 0))
    assert -1.0 <= draws.min() < -0.99 and 0.99 < draws.max() < 1.0 and abs(draws.mean()) < 0.05


# --------------------------------------------------------------------------------------------------- against truth
@pytest.mark.parametrize("name", P.TRUTH_CASES)
def test_restatement_against_truth(name):
    """The yardstick itself at 24 x 32, 3 views, 24 planes, radius 2, four iterations from the restated sweep's result.
    Median and 90th percentile of the inverse-depth error in plane spacings and the median angle of the normal to the true
    plane's, within 2 x the values measured when the test was written (patchmatch_cases.TRUTH_MEASURED):
        view 0 (22 degrees)   k = 0: 0.0970 / 6.3366 / 2.498 deg (sweep 0.6200 / 6.7531)   k = 0.08: 0.0860 / 6.2272 / 2.490 deg
        view 1 (12 degrees)   k = 0: 0.1111 / 0.3688 / 2.996 deg (sweep 0.3311 / 1.0456)   k = 0.08: 0.1043 / 0.3636 / 2.989 deg
        view 2 (2.3 degrees)  k = 0: 0.1332 / 2.1976 / 2.297 deg (sweep 0.1593 / 3.2028)   k = 0.08: 0.1255 / 2.3468 / 2.297 deg
    and, whatever those are, against the PARENT's result on the same case (the restated sweep): the refined median at most
    half the sweep's on views 0 and 1, not above it on view 2, the share of pixels with depth not below the sweep's."""
    case, ref = P.cases()[name], P.reference(name)
    assert case["iterations"] == 4 and case["num_planes"] == 24 and case["radius"] == 2 and case["frames"].shape == (3, 24, 32)
    depth, _, normal = ref["outs"][-1]
    (s_med, s_p90, s_valid), dw = P.sweep_errors(name)
    med, p90, valid = P.truth_errors(depth, P.truth_of(name), dw)
    angle = float(np.median(P.normal_angles(normal, depth > 0)))
    print(f"\n{name}: sweep median {s_med:.4f}, 90th percentile {s_p90:.4f}, valid {s_valid:.4f}; refined {med:.4f}, {p90:.4f}, "
          f"{valid:.4f}; median normal angle {angle:.3f} degrees")
    m_med, m_p90, m_angle = P.TRUTH_MEASURED[name]
    assert med <= 2 * m_med and p90 <= 2 * m_p90 and angle <= 2 * m_angle
    view = int(name[-1])
    assert med <= (0.5 * s_med if view in (0, 1) else s_med)
    assert valid >= s_valid


# --------------------------------------------------------------------------------------------------- structure
@pytest.mark.parametrize("name", ["k08_21x35", "holes", "normals", "wide_baseline"])
def test_a_step_never_raises_a_cost_and_leaves_the_other_colour(name):
    """The per-pixel cost after each half-iteration is <= the cost before it, exactly; a step of colour c leaves plane and
    cost of every pixel of colour 1 - c bit-identical; something is accepted; the stored cost is the cost of the stored plane."""
    states = P.reference(name)["states"]
    H, W = states[0][1].shape
    ys, xs = np.mgrid[0:H, 0:W]
    changed = 0
    for k in range(1, len(states)):
        colour = (k - 1) & 1
        other = ((xs + ys) & 1) != colour
        (p0, c0), (p1, c1) = states[k - 1], states[k]
        assert ((c1 <= c0) | (np.isinf(c0) & np.isinf(c1))).all()
        assert p1[other].tobytes() == p0[other].tobytes() and c1[other].tobytes() == c0[other].tobytes()
        changed += int((p1 != p0).any(-1).sum())
        assert ((c1 < c0) == (p1 != p0).any(-1)).all()                         # a plane changes exactly where its cost drops
    assert changed > 0
    again = P.plane_cost(P.reference(name)["ctx"], states[-1][0])
    assert again.tobytes() == states[-1][1].tobytes()


def test_seeds_iterations_and_the_start():
    """Two seeds give different planes; iterations = 0 returns the start; the fronto-parallel start has the sweep's costs;
    pixels without depth start inside the range; illegal normals fall back to the fronto-parallel plane."""
    case = P.cases()["holes"]
    a, b = P.reference("holes"), P.refine(dict(case, seed=case["seed"] + 1))
    assert a["states"][0][0].tobytes() != b["states"][0][0].tobytes()           # the holes are drawn by the seed
    assert a["states"][-1][0].tobytes() != b["states"][-1][0].tobytes()
    full = P.refine(dict(P.cases()["k08_24x32"], seed=1))
    assert full["states"][0][0].tobytes() == P.reference("k08_24x32")["states"][0][0].tobytes()      # no holes: the same start
    assert full["states"][-1][0].tobytes() != P.reference("k08_24x32")["states"][-1][0].tobytes()
    zero = P.refine(dict(case, iterations=0))
    assert len(zero["states"]) == 1 and zero["states"][0][0].tobytes() == a["states"][0][0].tobytes()
    hole = case["init_depth"] == 0
    start = a["states"][0][0]
    assert hole.any() and (start[..., :2] == 0).all()
    assert ((start[hole][:, 2] >= case["inv_depth_far"]) & (start[hole][:, 2] < case["inv_depth_near"])).all()
    assert np.array_equal(start[~hole][:, 2], 1.0 / case["init_depth"][~hole].astype(np.float64))
    kept = ~hole & (a["outs"][0][0] > 0)
    assert kept.any() and np.array_equal(a["outs"][0][0][kept], case["init_depth"][kept])   # 1 / (1 / z) rounds back to z
    # the sweep's cost volume at the chosen plane is the cost of the fronto-parallel plane (0, 0, w_j)
    from tests import mvs_cases as C
    sweep, sc = C.sweep_reference("k08_24x32"), P.cases()["k08_24x32"]
    ctx = P.reference("k08_24x32")["ctx"]
    for j in (0, 11, 23):
        plane = np.zeros(sc["frames"].shape[1:] + (3,))
        plane[..., 2] = sc["inv_depth_far"] + float(j) * sweep["dw"]
        assert P.plane_cost(ctx, plane).tobytes() == sweep["cost"][j].tobytes()
    nrm = P.cases()["normals"]
    given = (nrm["init_normals"] != 0).any(-1) & (nrm["init_depth"] > 0)
    slanted = (P.reference("normals")["states"][0][0][..., :2] != 0).any(-1)
    print(f"\nnormals: {int(given.sum())} given, {int(slanted.sum())} legal under {nrm['max_tilt_deg']} degrees")
    assert 0 < slanted.sum() < given.sum() and not (slanted & ~given).any()


# --------------------------------------------------------------------------------------------------- ties
def test_no_decision_of_a_gpu_case_is_a_tie():
    """The GPU tests exclude no pixel and compare plane bits, so in every case they use: the smallest |candidate cost -
    incumbent cost| over all legal, finite, unequal comparisons exceeds 100 x the order spread of this restatement (the
    tolerance of the GPU's costs); no legality test and no conf is closer to its threshold than that either (legality:
    patchmatch_cases.LEGALITY_MARGIN, relative).  Measured: spread 1.9e-14; gaps 6.0e-12 (k0_24x32, while the
    fronto-parallel start propagates) .. 4.2e-10; legality 1.5e-8 (range), 7.3e-5 (tilt); conf 4.3e-4."""
    spread = P.order_spread()
    print(f"\norder spread of the costs {spread:.3e}")
    assert 0 < spread < 1e-11
    for name in P.STEP_CASES + P.TRUTH_CASES:
        m = P.reference(name)["margins"]
        print(name, {k: f"{v:.2e}" for k, v in m.items()})
        assert m["gap"] > 100 * spread and m["conf"] > 100 * spread, (name, m)
        assert min(m["range"], m["tilt"], m["init_range"], m["init_tilt"]) > P.LEGALITY_MARGIN, (name, m)


def test_cases_cover_what_the_kernel_can_get_wrong():
    cases = {n: P.cases()[n] for n in P.STEP_CASES}
    assert {c["radius"] for c in cases.values()} == {1, 2, 3} and {len(c["sources"]) for c in cases.values()} >= {1, 2, 8}
    assert {c["frames"].shape[1:] for c in cases.values()} == {(24, 32), (21, 35)} and {c["min_views"] for c in cases.values()} == {1, 2}
    assert {float(c["cams"][0, 3]) for c in cases.values()} == {0.0, 0.08} and cases["M8"]["frames"].shape[0] == 9
    for name in ("facing_away", "constant_reference"):                       # all costs +inf: nothing is ever accepted
        states = P.reference(name)["states"]
        assert all(np.isinf(c).all() for _, c in states) and all(p.tobytes() == states[0][0].tobytes() for p, _ in states)
        assert all((d == 0).all() and (n == 0).all() and (c == 0).all() for d, c, n in P.reference(name)["outs"])
    wide = P.reference("wide_baseline")["states"][-1][1]
    assert np.isinf(wide).any() and np.isfinite(wide).any()
    assert (cases["holes"]["init_depth"] == 0).any() and cases["normals"]["init_normals"] is not None
    for name in P.STEP_CASES:                                                # every case accepts slanted planes, unless none can
        end = P.reference(name)["states"][-1][0]
        assert (end[..., :2] != 0).any() == (name not in ("facing_away", "constant_reference")), name
