"""The meshing kernels (vggsfm_amd/meshing.py, csrc/tsdf/tsdf.hip) against the NumPy restatement of tests/meshing_cases.py:
IDENTICAL BITS for the volumes, the edge masks, the offsets, the counts, the vertices, the colours, the normals and the
faces.  FP64 addition, multiplication, division and square root are correctly rounded on both sides, the library is built
without floating-point contraction and the kernels take every sum in the header's order, so nothing may differ;
tests/test_meshing_host.py asserts on the restatement that no decision of any case is closer than 1e-9 to a tie.  The
integration cases are 3 maps (one case: 258) of 24 x 32 or 21 x 35 into 21 x 17 x 13 or 9 x 7 x 5 nodes; the extraction cases
are volumes written directly, the largest 67 x 65 x 63 nodes (1072 groups: both levels of the count carry)."""
import numpy as np
import pytest
import torch

from tests import fusion_cases as FC
from tests import meshing_cases as C
from vggsfm_amd import meshing

pytestmark = pytest.mark.gpu

COUNT_KEYS = ("edge_mask", "vertex_offset", "face_offset", "group_counts", "group_offsets", "counts")


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _volume(case, color=None):
    color = (case.get("frames") is not None or case.get("rgb_sum") is not None) if color is None else color
    return meshing.TSDFVolume(case["origin"], case["voxel"], case["dims"], color=color)


def _integrate(vol, case, first=0, last=None):
    sl = slice(first, last)
    return vol.integrate(D(case["depth"][sl]), D(case["poses"][sl]), D(case["cams"][sl]), D(None if case["weights"] is None else
                                                                                             case["weights"][sl]),
                         D(None if case["frames"] is None else case["frames"][sl]), case["trunc"])


def _load(case):
    """a device volume holding the arrays of a case of meshing_cases.volume_cases()"""
    vol = _volume(case)
    vol.tsdf_sum.copy_(D(case["tsdf_sum"]))
    vol.weight_sum.copy_(D(case["weight_sum"]))
    if case["rgb_sum"] is not None:
        vol.rgb_sum.copy_(D(case["rgb_sum"]))
    return vol


def _assert_volumes_are(vol, ref, name):
    for k in ("tsdf_sum", "weight_sum", "rgb_sum"):
        got = getattr(vol, k)
        if ref[k] is None:
            assert got is None, (name, k)
            continue
        got = got.cpu().numpy()
        assert got.dtype == np.float64 and got.shape == ref[k].shape
        assert got.tobytes() == ref[k].tobytes(), (name, k, int((got != ref[k]).sum()))


def _assert_mesh_is(vol, ref, min_weight, name):
    """count and extract of a device volume against a reference of the restatement, bit for bit -> the mesh as NumPy arrays"""
    count = {k: v.cpu().numpy() for k, v in vol.count(min_weight).items()}
    for k in COUNT_KEYS:
        assert count[k].dtype == ref[k].dtype and count[k].shape == ref[k].shape, (name, k, count[k].dtype, count[k].shape)
        assert count[k].tobytes() == ref[k].tobytes(), (name, k, int((count[k] != ref[k]).sum()))
    mesh = vol.extract(min_weight)
    assert all(t.is_cuda for t in mesh)
    got = meshing.Mesh(*(t.cpu().numpy() for t in mesh))
    V, F = len(ref["vertices"]), len(ref["faces"])
    assert got.vertices.shape == got.normals.shape == got.rgb.shape == (V, 3) and got.faces.shape == (F, 3), name
    assert got.vertices.dtype == np.float64 and got.normals.dtype == got.rgb.dtype == np.float32 and got.faces.dtype == np.int32
    differ = int((got.normals != ref["normals"]).sum())
    print(f"\n{name}: {V} vertices, {F} faces; normal components that differ from the restatement: {differ}")
    for k in ("vertices", "rgb", "faces", "normals"):
        assert getattr(got, k).tobytes() == ref[k].tobytes(), (name, k, int((getattr(got, k) != ref[k]).sum()))
    return got


# --------------------------------------------------------------------------------------------------- integration
@pytest.mark.parametrize("name", list(C.integration_cases()))
def test_integration_and_mesh_match_restatement(name):
    case, ref = C.integration_cases()[name], C.integration_reference(name)
    vol = _integrate(_volume(case), case)
    _assert_volumes_are(vol, ref, name)
    got = _assert_mesh_is(vol, ref, case["min_weight"], name)
    if name == "all_zero":
        assert len(got.vertices) == 0 and len(got.faces) == 0
    else:
        n, _ = C.face_normals(got.vertices, got.faces)
        assert len(got.faces) > 0 and (n[:, 2] < 0).all()                      # every face looks at the cameras


def test_facing_away_adds_nothing_and_split_calls_add_up():
    """The view turned by 180 degrees leaves the volumes of the first two views; the views [0, 2) and then [2, 3) on the same
    volume give the bits of one call, with weights and colours."""
    away = C.integration_cases()["facing_away"]
    two = _integrate(_volume(away), away, 0, 2)
    three = _integrate(_volume(away), away)
    for k in ("tsdf_sum", "weight_sum", "rgb_sum"):
        assert torch.equal(getattr(two, k), getattr(three, k)), k
    for name in ("weights", "k08_21x35_small", "many_views"):
        case, ref = C.integration_cases()[name], C.integration_reference(name)
        cut = 2 if name != "many_views" else 100
        vol = _integrate(_integrate(_volume(case), case, 0, cut), case, cut, None)
        _assert_volumes_are(vol, ref, name)


def test_frames_without_colour_volume_and_colour_volume_without_frames():
    """frames given to a volume without colour are ignored; a colour volume integrated without frames keeps its colour sums
    and meshes with the colours it has (here: none, so the division 0 / w gives 0)."""
    case, ref = C.integration_cases()["k08_24x32"], C.integration_reference("k08_24x32")
    plain = _integrate(_volume(case, color=False), case)
    assert plain.rgb_sum is None and plain.tsdf_sum.cpu().numpy().tobytes() == ref["tsdf_sum"].tobytes()
    mesh = plain.extract(case["min_weight"])
    assert mesh.vertices.cpu().numpy().tobytes() == ref["vertices"].tobytes() and not mesh.rgb.any()
    keep = _volume(case, color=True)
    keep.integrate(D(case["depth"]), D(case["poses"]), D(case["cams"]), None, None, case["trunc"])
    assert not keep.rgb_sum.any() and torch.equal(keep.tsdf_sum, plain.tsdf_sum)
    again = keep.extract(case["min_weight"])
    assert torch.equal(again.faces, mesh.faces) and not again.rgb.any()


@pytest.mark.parametrize("name", C.TRUTH_CASES)
def test_kernel_against_the_true_plane(name):
    """The device's mesh within the CPU bounds of tests/test_meshing_host.py: 2 x the restatement's measured distances."""
    case = C.integration_cases()[name]
    mesh = _integrate(_volume(case), case).extract(case["min_weight"])
    dist = FC.plane_distance(mesh.vertices.cpu().numpy())
    print(f"\n{name}: distance to the plane: median {np.median(dist):.4e}, largest {dist.max():.4e}")
    assert len(dist) == 1353 and np.median(dist) <= 2 * C.TRUTH_MEDIAN and dist.max() <= 2 * C.TRUTH_LARGEST


# --------------------------------------------------------------------------------------------------- extraction
@pytest.mark.parametrize("name", list(C.volume_cases()))
def test_extraction_matches_restatement(name):
    case, ref = C.volume_cases()[name], C.volume_reference(name)
    got = _assert_mesh_is(_load(case), ref, case["min_weight"], name)
    top = C.topology(got.faces, len(got.vertices))
    if name in ("sphere", "sphere_no_colour", "two_spheres"):                  # closedness and Euler number on the device's mesh
        assert top["closed"] and top["euler"] == (4 if name == "two_spheres" else 2) and top["used"] == len(got.vertices)
    if name == "holes":
        assert not top["closed"] and top["duplicates"] == 0
    if name in ("all_inside", "all_outside"):
        assert len(got.vertices) == 0 and len(got.faces) == 0
    if name == "plane_67x65x63":
        assert len(ref["group_counts"]) > 1024


def test_the_sixteen_cases_on_the_device():
    """All 256 sign patterns of a 2 x 2 x 2 grid through the kernels: the faces of every pattern are the restatement's, which
    derives its table from the rule."""
    for pattern in range(0, 256, 1):
        case = C.sign_pattern_volume(pattern)
        mesh = _load(case).extract(case["min_weight"])
        ref = C.extract(**case)
        assert mesh.faces.cpu().numpy().tobytes() == ref["faces"].tobytes(), pattern
        assert mesh.vertices.cpu().numpy().tobytes() == ref["vertices"].tobytes(), pattern


def test_same_bits_twice_and_after_other_data():
    case, other = C.volume_cases()["holes"], C.volume_cases()["plane_67x65x63"]
    icase = C.integration_cases()["weights_zeros"]
    first = _load(case).extract(case["min_weight"])
    ivol = _integrate(_volume(icase), icase)
    _load(other).extract(other["min_weight"])
    _integrate(_volume(C.integration_cases()["k0_24x32"]), C.integration_cases()["k0_24x32"])
    again = _load(case).extract(case["min_weight"])
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    ivol2 = _integrate(_volume(icase), icase)
    for k in ("tsdf_sum", "weight_sum", "rgb_sum"):
        assert torch.equal(getattr(ivol, k), getattr(ivol2, k)), k
    vol = _load(case)
    for a, b in zip(vol.extract(case["min_weight"]), vol.extract(case["min_weight"])):   # the same volume twice
        assert torch.equal(a, b)


def test_a_row_beyond_the_capacity_is_not_written():
    """emit with room for fewer rows than counted: the rows below the capacity are the mesh's, nothing else is written."""
    case, ref = C.volume_cases()["sphere"], C.volume_reference("sphere")
    vol = _load(case)
    count = vol.count(case["min_weight"])
    part = vol.emit(count, 100, 200, case["min_weight"])
    assert part.vertices.cpu().numpy().tobytes() == ref["vertices"][:100].tobytes()
    assert part.faces.cpu().numpy().tobytes() == ref["faces"][:200].tobytes()
    assert part.normals.cpu().numpy().tobytes() == ref["normals"][:100].tobytes()
    assert part.rgb.cpu().numpy().tobytes() == ref["rgb"][:100].tobytes()
    none = vol.emit(count, 0, 0, case["min_weight"])
    assert none.vertices.shape == (0, 3) and none.faces.shape == (0, 3)


# --------------------------------------------------------------------------------------------------- the Python surface
def test_python_surface_defaults_and_refusals():
    case = C.integration_cases()["k08_24x32"]
    vol = _volume(case)
    depth, poses, cams = D(case["depth"]), D(case["poses"]), D(case["cams"])
    assert vol.integrate(depth, poses, cams) is vol                           # trunc defaults to 4 voxels
    want = C.integrate(case["depth"], None, None, case["poses"], case["cams"], case["origin"], case["voxel"], case["dims"],
                       4.0 * case["voxel"], *C.empty_volume(case["dims"], False))
    assert vol.tsdf_sum.cpu().numpy().tobytes() == want[0].tobytes() and not vol.rgb_sum.any()
    ref = C.extract(want[0], want[1], None, case["origin"], case["voxel"], case["dims"], 1.0)
    mesh = vol.extract()                                                      # min_weight defaults to 1
    assert mesh.faces.cpu().numpy().tobytes() == ref["faces"].tobytes() and len(ref["faces"]) > 0
    nan = float("nan")
    before = vol.tsdf_sum.clone()                                             # a refused call leaves the volume alone
    for bad in (dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=nan)):
        with pytest.raises(ValueError, match="trunc"):
            vol.integrate(depth, poses, cams, **bad)
    for bad in (0.0, -1.0, nan):
        with pytest.raises(ValueError, match="min_weight"):
            vol.extract(bad)
    with pytest.raises(ValueError, match="depth must be"):
        vol.integrate(depth.double(), poses, cams)
    with pytest.raises(ValueError, match="no view"):
        vol.integrate(depth[:0], poses[:0], cams[:0])
    with pytest.raises(ValueError, match="poses must be"):
        vol.integrate(depth, poses[:2], cams)
    with pytest.raises(ValueError, match="weights must be"):
        vol.integrate(depth, poses, cams, weights=depth[:, :-1])
    with pytest.raises(ValueError, match="frames must be"):
        vol.integrate(depth, poses, cams, frames=depth)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vol.integrate(depth.cpu(), poses, cams)
    assert torch.equal(before, vol.tsdf_sum)


def test_volume_bounds():
    g = torch.Generator().manual_seed(3)
    pts = torch.rand(5000, 3, generator=g, dtype=torch.float64) * torch.tensor([2.0, 1.0, 0.5]) + torch.tensor([1.0, -2.0, 3.0])
    pts[0] = torch.tensor([1e6, 1e6, -1e6])                                   # an outlier does not move the box
    origin, voxel, dims = meshing.volume_bounds(pts.cuda(), resolution=65, margin=0.05)
    lo, hi = np.percentile(pts.numpy(), 1, axis=0, method="lower"), np.percentile(pts.numpy(), 99, axis=0, method="higher")
    side = (hi - lo).max()
    assert dims[0] == 65 and dims[0] > dims[1] > dims[2] >= 2
    assert np.allclose(origin, lo - 0.05 * side) and np.isclose(voxel, 1.1 * side / 64)
    top = np.asarray(origin) + voxel * (np.asarray(dims) - 1)
    assert (top >= hi + 0.05 * side - 1e-9).all() and (top < hi + 0.05 * side + voxel).all()
    with pytest.raises(ValueError):
        meshing.volume_bounds(pts[:1].cuda().expand(4, 3))
    with pytest.raises(ValueError):
        meshing.volume_bounds(pts.cuda(), resolution=1)
