"""The multi-view stereo kernels (vggsfm_amd/mvs.py, csrc/mvs/mvs.hip) against the NumPy restatement of tests/mvs_cases.py.

Cost volume: the same pixels finite, and the finite costs within 100 x the spread between two runs of the restatement that
differ only in the order of the window sums (mvs_cases.sweep_order_spread: 4.7e-14 over the cases here, so 4.7e-12; the
factor is the tracker's, tests/test_gpu_klt.py).  FP64 division and square root are correctly rounded on both sides and
the kernel sums in the header's order, so little else can differ (measured on one MI355X: identical bits in every case).
Selection: index equal at every pixel (tests/test_mvs_host.py asserts on the restatement that no decision of any case is
closer than 1e-9 to a tie), depth and conf within one float32 step of the restatement's."""
import numpy as np
import pytest
import torch

from tests import mvs_cases as C
from vggsfm_amd import mvs

pytestmark = pytest.mark.gpu

SWEEP_CASES = list(C.sweep_cases()[0])


def D(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _sweep(case, return_cost=True, **over):
    c = dict(case, **over)
    return mvs.plane_sweep(D(c["frames"]), D(c["poses"]), D(c["cams"]), c["ref"], c["sources"], c["depth_near"], c["depth_far"],
                           c["num_planes"], c["radius"], c["min_views"], c["min_variance"], c["min_conf"],
                           return_cost=return_cost, rays=D(c["rays"]))


def _filter(case, **over):
    c = dict(case, **over)
    return mvs.filter_consistent(D(c["depth"]), D(c["poses"]), D(c["cams"]), c["ref"], c["sources"], c["rel_depth_tol"],
                                 c["reproj_tol"], c["min_consistent"], rays=D(c["rays"]), ray_index=c["ray_index"])


def _f32_step(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("name", SWEEP_CASES)
def test_sweep_matches_restatement(name):
    case, ref = C.sweep_cases()[0][name], C.sweep_reference(name)
    out = _sweep(case)
    depth, conf, index, cost = (t.cpu().numpy() for t in out)
    H, W = case["frames"].shape[1:]
    assert depth.shape == conf.shape == index.shape == (H, W) and cost.shape == (case["num_planes"], H, W)
    assert depth.dtype == conf.dtype == np.float32 and index.dtype == np.int32 and cost.dtype == np.float64
    finite = np.isfinite(ref["cost"])
    assert np.array_equal(np.isfinite(cost), finite) and np.isposinf(cost[~finite]).all()
    delta = np.abs(cost[finite] - ref["cost"][finite]).max(initial=0.0)
    tol = 100 * C.sweep_order_spread()
    print(f"\n{name}: max |delta cost| {delta:.3e} (tolerance {tol:.3e}), {int((index >= 0).sum())} of {index.size} pixels valid")
    assert delta <= tol
    assert np.array_equal(index, ref["index"])
    assert (np.abs(depth.astype(np.float64) - ref["depth"]) <= _f32_step(ref["depth"])).all()
    assert (np.abs(conf.astype(np.float64) - ref["conf"]) <= _f32_step(ref["conf"])).all()
    assert (depth[index < 0] == 0).all() and (depth[index >= 0] > 0).all() and np.isfinite(conf).all()
    if name in ("facing_away", "constant_reference"):
        assert (depth == 0).all() and (index == -1).all() and (conf == 0).all()


@pytest.mark.parametrize("name", ["k08_21x35", "wide_baseline"])
def test_sweep_without_cost_volume_gives_the_same_bits(name):
    case = C.sweep_cases()[0][name]
    with_cost, without = _sweep(case), _sweep(case, return_cost=False)
    assert without.cost is None
    for a, b in zip(with_cost[:3], without[:3]):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_sweep_is_deterministic_and_keeps_no_state():
    """The same call twice, and again after a call with the sources permuted: the same bits."""
    case = C.sweep_cases()[0]["wide_baseline"]
    first = [t.cpu().numpy() for t in _sweep(case)]
    second = [t.cpu().numpy() for t in _sweep(case)]
    permuted = [t.cpu().numpy() for t in _sweep(case, sources=case["sources"][::-1])]
    third = [t.cpu().numpy() for t in _sweep(case)]
    for a, b, c in zip(first, second, third):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert np.array_equal(np.isfinite(permuted[3]), np.isfinite(first[3]))            # the same sources are valid
    assert np.abs(permuted[3][np.isfinite(first[3])] - first[3][np.isfinite(first[3])]).max() < 1e-12


@pytest.mark.parametrize("name", list(C.filter_cases()))
def test_filter_matches_restatement(name):
    case, ref = C.filter_cases()[name], C.filter_reference(name)
    depth, count = (t.cpu().numpy() for t in _filter(case))
    assert depth.dtype == np.float32 and count.dtype == np.int32 and depth.shape == count.shape == case["depth"].shape[1:]
    print(f"\n{name}: counts {np.bincount(count.ravel()).tolist()}, kept {int((depth > 0).sum())}")
    assert np.array_equal(count, ref["count"]) and depth.tobytes() == ref["depth"].tobytes()
    again = [t.cpu().numpy() for t in _filter(case)]
    assert again[0].tobytes() == depth.tobytes() and again[1].tobytes() == count.tobytes()


@pytest.mark.parametrize("name", list(C.sweep_cases()[1]))
def test_sweep_against_truth(name):
    """The kernel on the analytic scene under the bound of tests/test_mvs_host.py::test_restatement_against_truth."""
    case, truth = C.sweep_cases()[0][name], C.sweep_cases()[1][name]
    out = _sweep(case, return_cost=False)
    got = {"depth": out.depth.cpu().numpy(), "index": out.index.cpu().numpy(), "dw": C.sweep_reference(name)["dw"]}
    med, p90, valid = C.truth_errors(got, truth)
    print(f"\n{name}: median {med:.4f}, 90th percentile {p90:.4f} plane spacings, valid {valid:.4f}")
    assert med <= 2 * C.TRUTH_MEDIAN and p90 <= 2 * C.TRUTH_P90 and 1.0 - valid <= 2 * C.TRUTH_INVALID


def test_python_surface_rays_and_defaults():
    """pixel_rays (cam_from_img on the pixel grid) against the closed form / Newton of the restatement, and the entries
    with the ray maps they derive themselves.  k = 0 is a subtraction and a division; under distortion the project's
    iterative undistortion stops once its step is shorter than 1e-5 (|step|^2 < 1e-10), which bounds what it can differ by
    from the converged value (measured: 4.9e-6, 2e-4 px at this focal length).  The entries run on such rays agree with the
    runs on the converged rays except where a decision is closer to its threshold than that."""
    for k, tol in ((0.0, 1e-15), (0.08, 1e-5)):
        cam = np.array([43.75, 17.3, 9.8, k])
        rays = mvs.pixel_rays(cam, 21, 35).cpu().numpy()
        assert rays.shape == (21, 35, 2) and rays.dtype == np.float64
        assert np.abs(rays - C.pixel_rays(cam, 21, 35)).max() <= tol
    case = C.filter_cases()["holes_mc2"]
    out = mvs.filter_consistent(D(case["depth"]), D(case["poses"]), D(case["cams"]), case["ref"], case["sources"])
    assert (out.count.cpu().numpy() == C.filter_reference("holes_mc2")["count"]).mean() > 0.99
    sweep = C.sweep_cases()[0]["k08_24x32"]
    got = mvs.plane_sweep(D(sweep["frames"]), D(sweep["poses"]), D(sweep["cams"]), sweep["ref"], sweep["sources"],
                          sweep["depth_near"], sweep["depth_far"], num_planes=24, min_variance=1e-5)
    assert got.cost is None and (got.index.cpu().numpy() == C.sweep_reference("k08_24x32")["index"]).mean() > 0.99


def test_every_refusal_raises():
    case = C.sweep_cases()[0]["k0_24x32"]
    invalid = "invalid argument"
    for over in (dict(num_planes=0), dict(num_planes=1025), dict(radius=0), dict(radius=4), dict(sources=[]),
                 dict(sources=list(range(9))), dict(min_views=0), dict(min_views=3), dict(ref=3), dict(ref=-1),
                 dict(sources=[0, 3]), dict(sources=[0, -1]), dict(sources=[0, 1]), dict(depth_near=5.0, depth_far=3.2),
                 dict(depth_near=4.0, depth_far=4.0)):
        with pytest.raises(RuntimeError, match=invalid):
            _sweep(case, **over)
    for over in (dict(depth_near=0.0), dict(depth_far=float("inf")), dict(depth_near=-1.0), dict(depth_far=float("nan"))):
        with pytest.raises(ValueError):
            _sweep(case, **over)
    with pytest.raises(ValueError):
        _sweep(case, rays=case["rays"][:-1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        mvs.plane_sweep(torch.from_numpy(case["frames"]), D(case["poses"]), D(case["cams"]), 1, [0, 2], 3.2, 5.0)
    flt = C.filter_cases()["holes_mc2"]
    for over in (dict(min_consistent=0), dict(ref=3), dict(sources=[1, 0]), dict(sources=[0, 5]), dict(sources=[]),
                 dict(ray_index=[0, 1, 0]), dict(rel_depth_tol=-0.01), dict(reproj_tol=float("nan"))):
        with pytest.raises(RuntimeError, match=invalid):
            _filter(flt, **over)
    with pytest.raises(ValueError):
        _filter(flt, ray_index=[0, 0])
