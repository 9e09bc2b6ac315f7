"""The depth-map fusion kernels (vggsfm_amd/fusion.py, csrc/fuse/fuse.hip) against the NumPy restatement of
tests/fusion_cases.py: IDENTICAL BITS for the normals, the `claimed` maps after the last view, the counts, view, pixel,
num_views, xyz, normals and colours.  FP64 addition, multiplication, division and square root are correctly rounded on both
sides, the library is built without floating-point contraction and the kernels take every sum in the header's order, so
nothing may differ; tests/test_fusion_host.py asserts on the restatement that no decision of any case is closer than 1e-9 to
a tie.  Each case is 3 (or 9) maps of 24 x 32 or 21 x 35."""
import numpy as np
import pytest
import torch

from tests import fusion_cases as C
from vggsfm_amd import fusion

pytestmark = pytest.mark.gpu

FIELDS = fusion.FusedCloud._fields


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _normals(case, **over):
    c = dict(case, **over)
    return fusion.depth_normals(D(c["depth"]), D(c["poses"]), np.zeros((len(c["depth"]), 4)), c["max_rel_jump"],
                                rays=D(c["rays"]), ray_index=c["ray_index"])


def _fuse(case, **over):
    """-> (cloud as NumPy arrays, claimed) of a case of fusion_cases (its normal map and colours given, not derived)"""
    c = dict(case, **over)
    angle = c.pop("max_normal_angle_deg", C.MAX_ANGLE_DEG)
    cloud, claimed = fusion.fuse_depth_maps(D(c["depth"]), D(c["poses"]), D(c["cams"]), c["sources"], D(c["colors"]),
                                            D(c["normals"]), c["rel_depth_tol"], c["reproj_tol"], angle, c["min_views"],
                                            c["view_order"], rays=D(c["rays"]), ray_index=c["ray_index"], return_claimed=True)
    assert all(t.is_cuda for t in cloud) and claimed.is_cuda
    return fusion.FusedCloud(*(t.cpu().numpy() for t in cloud)), claimed.cpu().numpy()


def _assert_cloud_is(cloud, claimed, ref, name):
    n = len(ref["xyz"])
    assert [len(a) for a in cloud] == [n] * 6, (name, [len(a) for a in cloud], n)
    assert cloud.xyz.dtype == np.float64 and cloud.normal.dtype == cloud.rgb.dtype == np.float32
    assert cloud.num_views.dtype == cloud.view.dtype == cloud.pixel.dtype == np.int32 and claimed.dtype == np.uint8
    assert cloud.xyz.shape == cloud.normal.shape == cloud.rgb.shape == (n, 3)
    assert np.array_equal(claimed, ref["claimed"]), name
    for k in ("view", "pixel", "num_views", "xyz", "normal", "rgb"):
        got, want = getattr(cloud, k), ref[k]
        assert got.tobytes() == want.tobytes(), (name, k, int((got != want).sum()))


def test_min_normal_cos_is_the_restatements():
    import math
    assert math.cos(math.radians(C.MAX_ANGLE_DEG)) == C.normal_cos()


@pytest.mark.parametrize("name", list(C.normals_cases()))
def test_normals_match_restatement(name):
    case, ref = C.normals_cases()[name], C.normals_reference(name)["normals"]
    got = _normals(case).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == case["depth"].shape + (3,)
    none = ~C._nonzero(got)
    print(f"\n{name}: {int(none.sum())} of {none.size} pixels without a normal, {int((got != ref).sum())} values differ")
    assert got.tobytes() == ref.tobytes()
    assert np.array_equal(none, ~C._nonzero(ref)) and (none[case["depth"] == 0]).all()
    norm = np.linalg.norm(got.astype(np.float64), axis=-1)
    assert np.abs(norm[~none] - 1.0).max(initial=0.0) < 1e-6


@pytest.mark.parametrize("name", ["k0_24x32", "k08_24x32"])
def test_normals_against_truth(name):
    """The kernel under the bound of tests/test_fusion_host.py::test_restatement_against_truth."""
    got = _normals(C.normals_cases()[name]).cpu().numpy()
    angle = C.normal_angle_deg(got)
    print(f"\n{name}: largest angle to the plane's normal {np.nanmax(angle):.4e} deg")
    assert not np.isnan(angle).any() and np.nanmax(angle) <= 2 * C.TRUTH_NORMAL_ANGLE_DEG


@pytest.mark.parametrize("name", list(C.fusion_cases()))
def test_fusion_matches_restatement(name):
    case, ref = C.fusion_cases()[name], C.fusion_reference(name)
    cloud, claimed = _fuse(case)
    print(f"\n{name}: {len(cloud.xyz)} points (restatement {len(ref['xyz'])}), per view {np.bincount(cloud.view, minlength=len(case['depth'])).tolist()}, "
          f"claimed {claimed.sum(axis=(1, 2)).tolist()}")
    _assert_cloud_is(cloud, claimed, ref, name)
    if name == "all_zero":
        assert cloud.xyz.shape == cloud.normal.shape == cloud.rgb.shape == (0, 3) and not claimed.any()
    if name == "copy_of_view0":
        assert claimed[1].all() and not (cloud.view == 1).any()
    if name == "off_mv2":
        assert not (cloud.view == 2).any()
    if name in C.TRUTH_CASES:
        dist = C.plane_distance(cloud.xyz).max()
        print(f"largest distance from the plane {dist:.4e}")
        assert dist <= 2 * C.TRUTH_PLANE_DISTANCE and np.nanmax(C.normal_angle_deg(cloud.normal)) <= 2 * C.TRUTH_NORMAL_ANGLE_DEG


def test_view_order_changes_the_cloud():
    a, _ = _fuse(C.fusion_cases()["order_201"])
    b, _ = _fuse(C.fusion_cases()["order_012"])
    assert len(a.xyz) != len(b.xyz) and a.view[0] == 2 and b.view[0] == 0
    assert a.xyz.tobytes() == C.fusion_reference("order_201")["xyz"].tobytes()
    assert b.xyz.tobytes() == C.fusion_reference("order_012")["xyz"].tobytes()


def test_fusion_is_deterministic_and_keeps_no_state():
    """The same call twice, and again after a call on other data: the same bits."""
    case = C.fusion_cases()["holes"]
    first = _fuse(case)
    second = _fuse(case)
    _fuse(C.fusion_cases()["nine_views"])
    _normals(C.normals_cases()["k08_21x35"])
    third = _fuse(case)
    for other in (second, third):
        assert other[1].tobytes() == first[1].tobytes()
        for a, b in zip(first[0], other[0]):
            assert a.tobytes() == b.tobytes()
    n1 = _normals(C.normals_cases()["holes"]).cpu().numpy()
    _normals(C.normals_cases()["depth_step"])
    assert _normals(C.normals_cases()["holes"]).cpu().numpy().tobytes() == n1.tobytes()


def test_python_surface_and_defaults():
    """normals="auto" derives the map the restatement derives, the default rays are mvs.camera_rays' (k = 0: the closed form
    of the restatement to 1e-15, so the counts agree), defaults as the issue names them."""
    case = C.fusion_cases()["k0_mv2"]
    cloud = fusion.fuse_depth_maps(D(case["depth"]), D(case["poses"]), D(case["cams"]), case["sources"], D(case["colors"]))
    ref = C.fusion_reference("k0_mv2")
    assert isinstance(cloud, fusion.FusedCloud) and abs(len(cloud.xyz) - len(ref["xyz"])) <= 2
    auto = fusion.fuse_depth_maps(D(case["depth"]), D(case["poses"]), D(case["cams"]), case["sources"], D(case["colors"]),
                                  rays=D(case["rays"]), ray_index=case["ray_index"])
    _assert_cloud_is(fusion.FusedCloud(*(t.cpu().numpy() for t in auto)), ref["claimed"], ref, "auto")
    none = fusion.fuse_depth_maps(D(case["depth"]), D(case["poses"]), D(case["cams"]), case["sources"], normals=None,
                                  rays=D(case["rays"]), ray_index=case["ray_index"])
    assert not none.normal.any() and not none.rgb.any() and none.normal.shape == none.rgb.shape == (len(none.xyz), 3)
    nrm = fusion.depth_normals(D(case["depth"]), D(case["poses"]), D(case["cams"]))
    assert nrm.shape == (3, 24, 32, 3) and (nrm.cpu().numpy() == case["normals"]).mean() > 0.99


def test_every_refusal_raises():
    case = C.fusion_cases()["k08_mv2"]
    invalid = "invalid argument"
    for over in (dict(sources=[[0], [0, 2], [0, 1]]), dict(sources=[[1, 3], [0, 2], [0, 1]]), dict(sources=[[1, -1], [0, 2], [0, 1]]),
                 dict(sources=[list(range(1, 10)), [0], [0]]), dict(min_views=0), dict(min_views=4), dict(min_views=-1),
                 dict(sources=[[], [], []]), dict(rel_depth_tol=-0.01), dict(rel_depth_tol=float("nan")), dict(reproj_tol=-1.0),
                 dict(reproj_tol=float("nan")), dict(ray_index=[0, 1, 0]), dict(ray_index=[0, 0, -1]), dict(view_order=[0, 3]),
                 dict(view_order=[-1])):
        with pytest.raises(RuntimeError, match=invalid):
            _fuse(case, **over)
    for over in (dict(ray_index=[0, 0]), dict(sources=[[1], [0]]), dict(view_order=[0, 0]), dict(max_normal_angle_deg=-1.0),
                 dict(max_normal_angle_deg=float("nan")), dict(normals=case["normals"][:2]), dict(colors=case["colors"][:, :2])):
        with pytest.raises(ValueError):
            _fuse(case, **over)
    ncase = C.normals_cases()["k08_24x32"]
    for over in (dict(max_rel_jump=-0.05), dict(max_rel_jump=float("nan")), dict(ray_index=[0, 1, 0]), dict(ray_index=[-1, 0, 0])):
        with pytest.raises(RuntimeError, match=invalid):
            _normals(ncase, **over)
    with pytest.raises(ValueError):
        _normals(ncase, ray_index=[0, 0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        fusion.depth_normals(torch.from_numpy(ncase["depth"]), ncase["poses"], np.zeros((3, 4)))
