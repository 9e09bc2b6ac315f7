"""CPU tests of the rasteriser: what its C-ABI registry has of its own (the registry itself is tests/test_side_libraries.py's),
what the entries refuse, the yardstick of the GPU tests (the NumPy restatement of tests/render_cases.py, which tests every
pixel against every face) against analytic truth, the candidate box the header gives the kernel against the pixels the
restatement finds covered, and the margins of every decision the GPU tests compare exactly.  No kernel is called here."""
import re

import numpy as np
import pytest

from tests import meshing_cases as MC
from tests import render_cases as C
from tests.test_c_abi import _parse_header
from vggsfm_amd import _lib_raster

NAMES = ["vggz_build_arch", "vggz_raster", "vggz_resolve", "vggz_point_visibility"]


# --------------------------------------------------------------------------------------------------- registry
def test_header_table_and_library_agree():
    """What only the rasteriser has (tests/test_side_libraries.py compares table, header and symbols): the names and
    prototypes pinned by hand, and the header's constants against the binding and the restatement."""
    header = open(_lib_raster.HEADER_PATH).read()
    functions, _ = _parse_header(header)
    assert list(_lib_raster.SIGNATURES) == list(functions) == NAMES
    assert functions["vggz_build_arch"] == ("pointer", [])
    assert functions["vggz_raster"] == ("int", ["pointer", "int", "pointer", "int", "int"] + ["pointer"] * 4 + ["int"] * 4 +
                                        ["double", "pointer", "pointer"])
    assert functions["vggz_resolve"][1] == ["pointer", "pointer", "int", "pointer", "int"] + ["pointer"] * 5 + ["int"] * 4 + \
        ["pointer"] * 6
    assert functions["vggz_point_visibility"][1] == ["pointer", "int"] + ["pointer"] * 3 + ["int"] * 3 + ["double", "pointer", "pointer"]
    consts = dict(re.findall(r"#define VGGZ_(\w+) (\d+)", header))
    assert [int(consts[k]) for k in ("MAX_VIEWS", "SOLO_PIXELS")] == [_lib_raster.MAX_VIEWS, _lib_raster.SOLO_PIXELS] == \
        [256, C.SOLO_PIXELS]


# --------------------------------------------------------------------------------------------------- refusals
def test_host_refusals_need_no_device():
    """What the entries refuse is decided on the host, before any launch (NULL pointers throughout): every out-of-range
    argument returns VGG_ERR_INVALID_ARGUMENT, the no-ops return VGG_OK, and Python refuses the same arguments first."""
    import ctypes

    L = _lib_raster.lib()
    nan = float("nan")
    ridx = (ctypes.c_int32 * 3)(0, 1, 0)
    good = dict(V=5, F=4, base=0, ridx=ridx, NR=2, S=3, H=4, W=5, near=1e-6, tol=0.01)

    def raster(**kw):
        a = dict(good, **kw)
        return L.vggz_raster(None, a["V"], None, a["F"], a["base"], None, None, None, a["ridx"], a["NR"], a["S"], a["H"], a["W"],
                             a["near"], None, None)

    def resolve(**kw):
        a = dict(good, **kw)
        return L.vggz_resolve(None, None, a["V"], None, a["F"], None, None, None, None, a["ridx"], a["NR"], a["S"], a["H"], a["W"],
                              None, None, None, None, None, None)

    def visible(**kw):
        a = dict(good, **kw)
        return L.vggz_point_visibility(None, a["V"], None, None, None, a["S"], a["H"], a["W"], a["tol"], None, None)
    shared = (dict(S=0), dict(S=-1), dict(H=-1), dict(W=-1), dict(V=-1))
    views = (dict(NR=1), dict(NR=0), dict(ridx=None), dict(ridx=(ctypes.c_int32 * 3)(0, -1, 0)))
    for entry, refused, noop in (
            (raster, shared + views + (dict(near=0.0), dict(near=-1.0), dict(near=nan), dict(F=-1), dict(base=-1),
                                       dict(base=2 ** 31 - 4, F=4), dict(base=2 ** 31 - 1, F=1)), dict(F=0)),
            (resolve, shared + views + (dict(F=-1),), dict(H=0)),
            (visible, shared + (dict(tol=-0.01), dict(tol=nan)), dict(V=0))):
        assert entry() == -1, entry.__name__                                      # NULL pointers with work to do
        assert entry(**noop) == 0, entry.__name__
        for bad in refused:
            assert entry(**dict(noop, **bad)) == -1, (entry.__name__, bad)        # refused even where nothing would be done
    assert raster(H=0) == 0 and raster(W=0) == 0 and raster(V=0) == 0 and raster(F=0, base=2 ** 31 - 1) == 0
    assert raster(base=2 ** 31 - 5) == -1 and raster(F=0, base=2 ** 31 - 5) == 0  # (the first: NULL pointers)
    assert resolve(W=0) == 0 and resolve(V=0, F=0) == -1                          # an empty mesh still writes its maps

    import torch
    from vggsfm_amd import render
    with pytest.raises(RuntimeError, match="no CPU path"):
        render.new_keys(3, 4, 5, "cpu")
    for bad in ((0, 4, 5), (3, -1, 5)):
        with pytest.raises(ValueError, match="keys need"):
            render.new_keys(*bad)
    with pytest.raises(ValueError, match="keys must be"):
        render.rasterize(torch.zeros(3, 4, 5, dtype=torch.int32), None, None, None, None)
    with pytest.raises(ValueError, match="keys must be"):
        render.resolve(torch.zeros(4, 5, dtype=torch.int64), None, None, None, None)
    with pytest.raises(RuntimeError):
        render.rasterize(torch.zeros(3, 4, 5, dtype=torch.int64), None, None, None, None)        # keys on the host
    with pytest.raises(ValueError, match="rel_tol|depth must be"):
        render.visible_points(torch.zeros(2, 3), torch.zeros(3, 4, 5, dtype=torch.float64), None, None)


# --------------------------------------------------------------------------------------------------- against truth
@pytest.mark.parametrize("name", ["plane_k0", "plane_k08", "plane_km10", "plane_21x35", "plane_two_cams"])
def test_plane_has_no_hole_and_the_true_depth(name):
    """The jittered, row-shuffled grid covers every frame, so every pixel must be hit (the canonical edge direction leaves no
    crack), and the depth is the plane's along the pixel's ray to float32 rounding: |z - z_true| <= z 2^-23.  Permuting the
    faces leaves the depth map's bits unchanged (the face map then names the permuted rows)."""
    c, ref = C.cases()[name], C.reference(name)
    assert len(c["faces"]) == 128 and (ref["face"] >= 0).all() and (ref["depth"] > 0).all()
    worst = 0.0
    for s in range(3):
        true = C.plane_depth(c["poses"][s], c["rays"][c["ray_index"][s]])
        err = np.abs(ref["depth"][s].astype(np.float64) - true) / true
        worst = max(worst, float(err.max()))
    print(f"\n{name}: holes 0 of {ref['depth'].size}; largest |z - z_true| / z = {worst:.3e} (bound 2^-23 = {2.0 ** -23:.3e})")
    assert worst <= 2.0 ** -23
    assert np.abs(ref["weights"].sum(-1) - 1.0).max() < 1e-12 and ref["weights"].min() >= 0.0
    perm = np.random.default_rng(4).permutation(128)
    again = C.render(c["vertices"], c["faces"][perm], None, None, c["poses"], c["cams"], c["rays"], c["ray_index"], c["H"], c["W"])
    assert again["depth"].tobytes() == ref["depth"].tobytes()
    assert np.array_equal(perm[again["face"]], ref["face"])
    order = (c["faces"][:, 0] < c["faces"][:, 1]).mean()                      # the shuffle makes both edge directions occur
    assert 0.2 < order < 0.8


@pytest.mark.parametrize("name", ["sphere_k08", "sphere_21x35"])
def test_sphere_depth_is_the_nearer_root(name):
    """The 1 524-face sphere: a rendered point lies on a triangle whose vertices are within dv = 3 / (8 R) voxels of the sphere
    (tests/test_meshing_host.py) and whose edges are at most sqrt(3) voxels long, so its distance from the centre is within
    [R - dv - 3 / (8 (R - dv)), R + dv] (the chord bound L^2 / 8 R of section 32, scaled).  It is the FRONT hit: on a ray
    that enters the sphere of the lower bound it lies before that sphere; every such ray is hit and no ray that misses the
    sphere of the upper bound is."""
    c, ref = C.cases()[name], C.reference(name)
    assert len(c["faces"]) == 1524 and 1524 % 64 != 0
    R, scale = MC.SPHERE_RADIUS, C.SPHERE_SCALE
    dv = 3.0 / (8.0 * R)
    lo, hi = (R - dv - 3.0 / (8.0 * (R - dv))) * scale, (R + dv) * scale
    hits = 0
    for s in range(3):
        centre, d = C.pixel_world_rays(c["poses"][s], c["rays"][c["ray_index"][s]])
        z = ref["depth"][s].astype(np.float64)
        X = centre + z[..., None] * d
        rad = np.linalg.norm(X - C.SPHERE_AT, axis=-1)
        hit = z > 0
        hits += int(hit.sum())
        assert (rad[hit] >= lo - 1e-6).all() and (rad[hit] <= hi + 1e-6).all(), (rad[hit].min(), rad[hit].max(), lo, hi)
        u = d / np.linalg.norm(d, axis=-1, keepdims=True)
        oc = C.SPHERE_AT - centre
        miss = np.linalg.norm(oc - (oc * u).sum(-1)[..., None] * u, axis=-1)     # distance of the ray from the centre
        assert hit[miss < lo].all() and not hit[miss > hi].any()
        # the nearer root: along a ray that enters the inner sphere the surface lies before that sphere, not behind it
        along = ((X - C.SPHERE_AT) * u).sum(-1)
        inner = miss < lo
        assert (along[inner] <= -np.sqrt(lo * lo - miss[inner] ** 2) + 1e-9).all()
    print(f"\n{name}: {hits} pixels hit; radius of a rendered point within [{lo:.4f}, {hi:.4f}]")
    assert hits > 300
    n = ref["normal"].astype(np.float64)
    on = ref["face"] >= 0
    assert np.abs(np.linalg.norm(n[on], axis=-1) - 1.0).max() < 1e-6 and not n[~on].any() and not ref["rgb"][~on].any()


def test_occlusion_equal_depths_and_skipped_faces():
    c, ref = C.cases()["occluding_quads"], C.reference("occluding_quads")
    near_quad = ref["face"] >= 2
    far_quad = (ref["face"] == 0) | (ref["face"] == 1)
    assert near_quad.any() and far_quad.any() and ref["depth"][near_quad].max() < ref["depth"][far_quad].min()
    for s in range(3):                                   # the far quad covers the near one's pixels too, and loses them
        far, near = ref["covered"][s][:2].any(0).reshape(24, 32), ref["covered"][s][2:].any(0).reshape(24, 32)
        assert (far >= near).all() and np.array_equal(near, near_quad[s]) and np.array_equal(far & ~near, far_quad[s])
    twice = C.reference("same_face_twice")
    assert (twice["face"] == 0).sum() > 50 and not (twice["face"] == 1).any()       # equal depths: the lower index wins
    assert all(np.array_equal(cv[0], cv[1]) for cv in twice["covered"])
    for name in ("skippable", "skippable_21x35"):
        sk = C.reference(name)
        assert set(np.unique(sk["face"])) == {-1, 8}                                # only the good face is drawn
        assert all(not cv[[0, 1, 2, 3, 4, 5, 6, 7, 9, 10]].any() for cv in sk["covered"])
    assert (C.reference("one_face")["face"] == 0).any() and (C.reference("no_face")["face"] == -1).all()
    fill = C.reference("fill_k08")
    assert (fill["face"] >= 0).all() and set(np.unique(fill["face"])) == {0, 1}


def test_every_covered_pixel_lies_in_the_kernels_box():
    """The restatement has no box; the kernel's is the header's.  For every case, view and face: the pixels the restatement
    finds covered lie inside the box (fill_km10 included: two frame-filling triangles under k = -0.1).  The box-size case
    has, in its middle view, boxes of exactly 1, 63, 64, 65 and 690 pixels, 14 of each: both sides of the kernel's threshold
    and the threshold itself."""
    for name, c in C.cases().items():
        ref = C.reference(name)
        H, W = c["H"], c["W"]
        ys, xs = np.mgrid[0:H, 0:W]
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        for s in range(3):
            has, x0, x1, y0, y1 = C.face_box(c["vertices"], c["faces"], c["poses"][s], c["cams"][s], c["near"], H, W)
            cov = ref["covered"][s]
            assert not cov[~has].any(), (name, s)
            inside = (xs[None] >= x0[:, None]) & (xs[None] <= x1[:, None]) & (ys[None] >= y0[:, None]) & (ys[None] <= y1[:, None])
            assert not (cov & ~inside).any(), (name, s, np.nonzero((cov & ~inside).any(1))[0][:5])
            if name == "box_sizes" and s == 1:
                count = np.where(has, (x1 - x0 + 1) * (y1 - y0 + 1), 0)
                assert sorted(set(count.tolist())) == [1, 63, 64, 65, 690] and (np.bincount(count)[[1, 63, 64, 65, 690]] == 14).all()
                assert count[:5].tolist() == [1, 63, 64, 65, 690]                   # interleaved within a wavefront
                assert C.SOLO_PIXELS == 64 and len(count) == 70
                assert cov[count > 1].any(1).all() and not cov[count == 1].any()


def test_no_decision_of_a_gpu_case_is_a_tie():
    """The GPU tests compare bits, so no decision of a case they use may sit on its threshold: over all cases but the one that
    draws a face twice, the smallest nonzero |w_j| of any valid face at any pixel is > 1e-12 (an exact zero is decided
    identically by the two faces that share the edge, so it is allowed); the visibility case keeps the nearest-pixel rounding
    and |Xc[2] - z_r (1 + rel_tol)| away from ties."""
    worst = np.inf
    for name in C.TIE_FREE:
        m = C.reference(name)["margin"]
        print(name, f"{m:.3e}")
        assert m > 1e-12, (name, m)
        worst = min(worst, m)
    assert set(C.TIE_FREE) == set(C.cases()) - {"same_face_twice"}
    v = C.visibility_case()
    out, mg = C.point_visibility(v["points"], v["depth"], v["poses"], v["cams"], v["rel_tol"], detail=True)
    print({k: f"{x:.2e}" for k, x in mg.items()}, f"smallest |w| {worst:.3e}")
    assert mg["round"] > 1e-9 and mg["tol"] > 1e-9 and mg["front"] > 1e-9
    before, on, behind = out[1, 21:70], out[1, 70:130], out[1, 130:]         # as the middle camera sees them
    assert out.any() and not out.all() and not out[:, :21].any()             # behind the cameras, outside the frames, NaN
    # before it: all but those whose nearest pixel misses the silhouette; on it: part of the front half (the depth is the
    # nearest pixel's); behind it: none
    assert before.mean() > 0.7 and not behind.any() and 0.1 < on.mean() < 0.6


def test_cases_cover_what_the_kernel_can_get_wrong():
    cases = C.cases()
    assert {(c["H"], c["W"]) for c in cases.values()} == {(24, 32), (21, 35)}
    assert {float(c["cams"][0, 3]) for c in cases.values()} == {0.0, 0.08, -0.1}
    two = cases["plane_two_cams"]
    assert len(two["rays"]) == 2 and two["ray_index"].tolist() == [0, 1, 0] and (two["cams"][0] != two["cams"][1]).any()
    assert (21 * 35) % 256 != 0 and len(cases["box_sizes"]["faces"]) == 70 and len(cases["no_face"]["faces"]) == 0
    # split calls and two meshes in one buffer give the bits of one call, in the restatement too
    c, ref = cases["sphere_k08"], C.reference("sphere_k08")
    keys = np.full((3, 24, 32), C.EMPTY, np.uint64)
    args = (c["poses"], c["cams"], c["rays"], c["ray_index"], c["near"])
    keys = C.raster(keys, c["vertices"], c["faces"][700:], 700, *args)
    keys = C.raster(keys, c["vertices"], c["faces"][:700], 0, *args)
    assert keys.tobytes() == ref["keys"].tobytes()
