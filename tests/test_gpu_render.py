"""The rasteriser's kernels (vggsfm_amd/render.py, csrc/raster/raster.hip) against the NumPy restatement of
tests/render_cases.py, which tests every pixel against every face: IDENTICAL BITS for the keys, the depth, the face, the
weights, the normals and the colours.  FP64 addition, multiplication, division and square root are correctly rounded on
both sides, the library is built without floating-point contraction and the kernels evaluate the header's expressions in
the header's order, so nothing may differ; tests/test_render_host.py asserts on the restatement that no decision of any case
is a tie.  Every case is 3 views of 24 x 32 or 21 x 35 and at most 1 524 faces."""
import numpy as np
import pytest
import torch

from tests import meshing_cases as MC
from tests import render_cases as C
from vggsfm_amd import meshing, render

pytestmark = pytest.mark.gpu

MAPS = ("depth", "face", "weights", "normal", "rgb")


def D(x):
    return None if x is None else torch.from_numpy(np.array(x)).cuda()       # (a copy: the cases' arrays are read-only)


def _views(c):
    return dict(poses=D(c["poses"]), cams=D(c["cams"]), rays=D(c["rays"]), ray_index=c["ray_index"])


def _keys(c):
    return render.new_keys(len(c["poses"]), c["H"], c["W"])


def _raster(keys, c, faces=None, face_base=0, vertices=None):
    v = _views(c)
    return render.rasterize(keys, D(c["vertices"] if vertices is None else vertices), D(c["faces"] if faces is None else faces),
                            v["poses"], v["cams"], c["near"], face_base, v["rays"], v["ray_index"])


def _resolve(keys, c, normals=True, rgb=True, weights=True, faces=None, vertices=None, attrs=None):
    v = _views(c)
    n, col = (c["normals"], c["rgb"]) if attrs is None else attrs
    return render.resolve(keys, D(c["vertices"] if vertices is None else vertices), D(c["faces"] if faces is None else faces),
                          v["poses"], v["cams"], D(n) if normals else None, D(col) if rgb else None, weights, v["rays"],
                          v["ray_index"])


def _same(got, want, what):
    got = got.cpu().numpy()
    if got.dtype == np.int64 and want.dtype == np.uint64:
        got = got.view(np.uint64)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))


def _assert_render_is(keys, out, ref, name):
    _same(keys, ref["keys"], (name, "keys"))
    for k in MAPS:
        if k == "normal":
            differ = int((getattr(out, k).cpu().numpy() != ref[k]).sum())
            print(f"\n{name}: {int((ref['face'] >= 0).sum())} pixels hit; normal components that differ from the restatement: {differ}")
        _same(getattr(out, k), ref[k], (name, k))


# --------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("name", list(C.cases()))
def test_render_matches_restatement(name):
    c, ref = C.cases()[name], C.reference(name)
    keys = _raster(_keys(c), c)
    out = _resolve(keys, c)
    assert all(t.is_cuda for t in out) and keys.dtype == torch.int64
    _assert_render_is(keys, out, ref, name)
    if name == "no_face":
        assert bool((keys == -1).all())
    if name == "same_face_twice":
        assert not bool((out.face == 1).any()) and bool((out.face == 0).any())


def test_split_calls_two_meshes_and_permuted_faces():
    """[0, a) then [a, F) with face_base = a, in either order and with a inside a wavefront, give the bits of one call; two
    meshes drawn into one buffer give the bits of the concatenated mesh; permuted faces give the same depth bits."""
    c, ref = C.cases()["sphere_k08"], C.reference("sphere_k08")
    for a in (700, 1, 1523):
        keys = _raster(_raster(_keys(c), c, c["faces"][a:], a), c, c["faces"][:a], 0)
        _same(keys, ref["keys"], ("split", a))
    q, s = C.cases()["occluding_quads"], C.cases()["sphere_k08"]
    vertices = np.concatenate([q["vertices"], s["vertices"]])
    faces = np.concatenate([q["faces"], s["faces"] + len(q["vertices"])]).astype(np.int32)
    both = C.render(vertices, faces, None, None, q["poses"], q["cams"], q["rays"], q["ray_index"], 24, 32)
    keys = _raster(_keys(q), q)
    keys = _raster(keys, q, s["faces"], len(q["faces"]), s["vertices"])
    _same(keys, both["keys"], "two meshes")
    out = _resolve(keys, q, False, False, True, faces, vertices)
    _same(out.depth, both["depth"], "two meshes depth")
    _same(out.weights, both["weights"], "two meshes weights")
    perm = np.random.default_rng(4).permutation(len(c["faces"]))
    keys = _raster(_keys(c), c, c["faces"][perm])
    _same(_resolve(keys, c, False, False, False, c["faces"][perm]).depth, ref["depth"], "permuted")


def test_same_bits_twice_and_after_other_data():
    c, other = C.cases()["box_sizes"], C.cases()["plane_21x35"]
    first = _raster(_keys(c), c)
    out1 = _resolve(first, c)
    _resolve(_raster(_keys(other), other), other)
    again = _raster(_keys(c), c)
    out2 = _resolve(again, c)
    assert torch.equal(first, again)
    for a, b in zip(out1, out2):
        assert torch.equal(a, b)
    assert torch.equal(_raster(again.clone(), c), again)                     # drawn a second time onto itself: nothing falls


def test_outputs_off_touch_nothing_else():
    """Every combination of absent attributes and weights: what is given has the restatement's bits, what is not is None;
    a key that names a face beyond the faces given, or a face with a bad row, resolves as empty."""
    c, ref = C.cases()["plane_21x35"], C.reference("plane_21x35")
    keys = _raster(_keys(c), c)
    for normals in (False, True):
        for rgb in (False, True):
            for weights in (False, True):
                out = _resolve(keys, c, normals, rgb, weights)
                _same(out.depth, ref["depth"], "depth")
                _same(out.face, ref["face"], "face")
                for k, on in (("normal", normals), ("rgb", rgb), ("weights", weights)):
                    if on:
                        _same(getattr(out, k), ref[k], k)
                    else:
                        assert getattr(out, k) is None
    few = c["faces"][:50]
    want = C.resolve(ref["keys"], c["vertices"], few, c["normals"], c["rgb"], c["poses"], c["rays"], c["ray_index"])
    assert (want["face"] == -1).any() and (want["face"] >= 0).any()
    out = _resolve(keys, c, faces=few)
    for k in MAPS:
        _same(getattr(out, k), want[k], ("fewer faces", k))
    sk, skref = C.cases()["skippable"], C.reference("skippable")
    forged = skref["keys"].copy()                                            # keys that name the faces with bad rows
    forged[0, 0, :11] = (np.uint64(0x40000000) << np.uint64(32)) | np.arange(11, dtype=np.uint64)
    want = C.resolve(forged, sk["vertices"], sk["faces"], sk["normals"], sk["rgb"], sk["poses"], sk["rays"], sk["ray_index"])
    assert (want["face"][0, 0, [2, 4, 5, 9, 10]] == -1).all() and want["face"][0, 0, 8] == 8
    out = _resolve(D(forged.view(np.int64)), sk)
    for k in ("depth", "face"):
        _same(getattr(out, k), want[k], ("forged", k))
    hit = want["face"][0, 0, :11] == -1                                      # (a forged key off its face gives NaN weights)
    assert not out.weights[0, 0, :11][torch.from_numpy(hit).cuda()].any()


def test_visible_points_match_restatement():
    v = C.visibility_case()
    want = C.point_visibility(v["points"], v["depth"], v["poses"], v["cams"], v["rel_tol"])
    got = render.visible_points(D(v["points"]), D(v["depth"]), D(v["poses"]), D(v["cams"]), v["rel_tol"])
    assert got.dtype == torch.bool and got.shape == (3, 200) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want.astype(bool)) and want.any() and not want.all()
    loose = C.point_visibility(v["points"], v["depth"], v["poses"], v["cams"], 0.5)
    got = render.visible_points(D(v["points"]), D(v["depth"]), D(v["poses"]), D(v["cams"]), 0.5)
    assert np.array_equal(got.cpu().numpy(), loose.astype(bool)) and loose.sum() > want.sum()
    assert render.visible_points(D(v["points"][:0]), D(v["depth"]), D(v["poses"]), D(v["cams"])).shape == (3, 0)


def test_render_mesh_of_an_extracted_mesh_and_the_python_surface():
    """render_mesh of the Mesh that TSDFVolume.extract gives on the 9 x 7 x 5 integration case of the meshing tests: the bits
    of the restatement on that mesh read back; bare tensors and the defaults (ray maps from mvs.camera_rays) agree."""
    case = MC.integration_cases()["k08_21x35_small"]
    vol = meshing.TSDFVolume(case["origin"], case["voxel"], case["dims"])
    vol.integrate(D(case["depth"]), D(case["poses"]), D(case["cams"]), None, D(case["frames"]), case["trunc"])
    mesh = vol.extract(case["min_weight"])
    assert mesh.faces.shape[0] > 0
    from vggsfm_amd import mvs
    rays, ridx = mvs.camera_rays(D(case["cams"]), 21, 35)
    host = [t.cpu().numpy() for t in mesh]
    want = C.render(host[0], host[3], host[1], host[2], case["poses"], case["cams"], rays.cpu().numpy(), ridx.numpy(), 21, 35)
    assert (want["face"] >= 0).sum() > 100
    out = render.render_mesh(mesh, poses=D(case["poses"]), cams=D(case["cams"]), height=21, width=35, return_weights=True)
    for k in MAPS:
        _same(getattr(out, k), want[k], ("render_mesh", k))
    bare = render.render_mesh(mesh.vertices, mesh.faces, poses=D(case["poses"]), cams=D(case["cams"]), height=21, width=35,
                              normals=mesh.normals, colors=None)
    assert torch.equal(bare.depth, out.depth) and torch.equal(bare.normal, out.normal) and bare.rgb is None and bare.weights is None
    plain = render.render_mesh(mesh, poses=D(case["poses"]), cams=D(case["cams"]), height=21, width=35, normals=False, colors=False)
    assert plain.normal is None and plain.rgb is None and torch.equal(plain.face, out.face)
    nan = float("nan")
    keys = render.new_keys(3, 21, 35)
    for bad in (0.0, -1.0, nan):
        with pytest.raises(ValueError, match="near"):
            render.rasterize(keys, mesh.vertices, mesh.faces, D(case["poses"]), D(case["cams"]), near=bad)
    with pytest.raises(ValueError, match="face_base"):
        render.rasterize(keys, mesh.vertices, mesh.faces, D(case["poses"]), D(case["cams"]), face_base=-1)
    with pytest.raises(ValueError, match="face_base"):
        render.rasterize(keys, mesh.vertices, mesh.faces, D(case["poses"]), D(case["cams"]), face_base=2 ** 31 - 5)
    with pytest.raises(ValueError, match="faces must be"):
        render.rasterize(keys, mesh.vertices, mesh.faces.long(), D(case["poses"]), D(case["cams"]))
    with pytest.raises(ValueError, match="poses must be"):
        render.rasterize(keys, mesh.vertices, mesh.faces, D(case["poses"][:2]), D(case["cams"]))
    with pytest.raises(ValueError, match="ray_index"):
        render.rasterize(keys, mesh.vertices, mesh.faces, D(case["poses"]), D(case["cams"]), rays=rays, ray_index=[0, 1, 0])
    with pytest.raises(ValueError, match="normals must be"):
        render.resolve(keys, mesh.vertices, mesh.faces, D(case["poses"]), D(case["cams"]), normals=mesh.normals[:-1])
    with pytest.raises(ValueError, match="rel_tol"):
        render.visible_points(mesh.vertices, out.depth, D(case["poses"]), D(case["cams"]), rel_tol=-0.1)
    assert bool((keys == -1).all())                                          # a refused call leaves the keys alone
    empty = render.render_mesh(mesh.vertices[:0], mesh.faces[:0], poses=D(case["poses"]), cams=D(case["cams"]), height=21, width=35,
                               normals=mesh.normals[:0], colors=mesh.rgb[:0], return_weights=True)
    assert bool((empty.face == -1).all()) and not empty.depth.any() and not empty.normal.any() and not empty.rgb.any() \
        and not empty.weights.any()
