"""The PatchMatch kernels (vggsfm_amd/patchmatch.py, csrc/patchmatch/patchmatch.hip) against the NumPy restatement of
tests/patchmatch_cases.py.

plane_cost of the fronto-parallel planes (0, 0, w_j): the bits of the sweep's cost volume, which ties the new arithmetic to
the old.  Then the state after plane_init, plane_cost and EVERY half-iteration: plane bits, depth, normal and the finite
pattern of the cost identical, cost and conf within 100 x the spread between two runs of the restatement that differ only in
the order of the window sums (patchmatch_cases.order_spread: 1.9e-14, so 1.9e-12; tests/test_patchmatch_host.py asserts on
the restatement that no decision of any case is closer than that to a tie).  FP64 division and square root are correctly
rounded on both sides and the kernel sums in the header's order, so little else can differ."""
import numpy as np
import pytest
import torch

from tests import mvs_cases as C
from tests import patchmatch_cases as P
from vggsfm_amd import fusion, mvs
from vggsfm_amd import patchmatch as PM

pytestmark = pytest.mark.gpu


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _device(case):
    return dict(frames=D(case["frames"]), poses=D(case["poses"]), cams=D(case["cams"]), rays=D(case["rays"]))


def _start(case, dev):
    plane = PM.plane_init(D(case["init_depth"]), dev["poses"], case["ref"], dev["rays"], case["depth_near"], case["depth_far"],
                          D(case["init_normals"]), case["max_tilt_deg"], case["seed"])
    cost = PM.plane_cost(dev["frames"], dev["poses"], dev["cams"], case["ref"], case["sources"], plane, case["radius"],
                         case["min_views"], case["min_variance"], dev["rays"])
    return plane, cost


def _step(case, dev, plane, cost, iteration, colour):
    PM.step(dev["frames"], dev["poses"], dev["cams"], case["ref"], case["sources"], plane, cost, case["depth_near"],
            case["depth_far"], iteration, colour, case["depth_step"], case["slope_step"], case["max_tilt_deg"], case["radius"],
            case["min_views"], case["min_variance"], case["seed"], dev["rays"])


def _refine(case, **over):
    c = dict(case, **over)
    return PM.refine_depth(D(c["frames"]), D(c["poses"]), D(c["cams"]), c["ref"], c["sources"], c["depth_near"], c["depth_far"],
                           D(c["init_depth"]), D(c["init_normals"]), c["iterations"], c["radius"], c["min_views"],
                           c["min_variance"], c["min_conf"], c["seed"], c["depth_step"], c["slope_step"], c["max_tilt_deg"],
                           D(c["rays"]), c["num_planes"])


@pytest.mark.parametrize("name", ["k08_24x32", "k08_21x35", "M8"])
def test_plane_cost_of_fronto_parallel_planes_is_the_sweeps_cost_volume(name):
    """(0, 0, w_j) for j = 0, 11 and 23: plane_cost equals plane_sweep(..., return_cost=True).cost[j] bit for bit."""
    case = C.sweep_cases()[0][name]
    dev = _device(case)
    sweep = mvs.plane_sweep(dev["frames"], dev["poses"], dev["cams"], case["ref"], case["sources"], case["depth_near"],
                            case["depth_far"], case["num_planes"], case["radius"], case["min_views"], case["min_variance"],
                            case["min_conf"], return_cost=True, rays=dev["rays"])
    volume = sweep.cost.cpu().numpy()
    H, W = case["frames"].shape[1:]
    dw = (case["inv_depth_near"] - case["inv_depth_far"]) / float(case["num_planes"] - 1)
    for j in (0, 11, 23):
        plane = np.zeros((H, W, 3))
        plane[..., 2] = case["inv_depth_far"] + float(j) * dw
        got = PM.plane_cost(dev["frames"], dev["poses"], dev["cams"], case["ref"], case["sources"], D(plane), case["radius"],
                            case["min_views"], case["min_variance"], dev["rays"]).cpu().numpy()
        print(f"\n{name} plane {j}: {int(np.isfinite(got).sum())} of {got.size} costs finite, "
              f"{int((got != volume[j]).sum())} differ from the sweep's")
        assert got.dtype == np.float64 and got.shape == (H, W) and np.isfinite(got).any()
        assert got.tobytes() == volume[j].tobytes()


@pytest.mark.parametrize("name", P.STEP_CASES)
def test_every_half_iteration_matches_restatement(name):
    case, ref = P.cases()[name], P.reference(name)
    tol = 100 * P.order_spread()
    dev = _device(case)
    pose, H, W = case["poses"][case["ref"]], *case["frames"].shape[1:]
    plane, cost = _start(case, dev)
    worst = 0.0

    def check(k):
        nonlocal worst
        depth, conf, normal = (t.cpu().numpy() for t in PM.outputs(plane, cost, dev["poses"], case["ref"], dev["rays"], case["min_conf"]))
        p, c = plane.cpu().numpy(), cost.cpu().numpy()
        rp, rc = ref["states"][k]
        rd, rconf, rn = ref["outs"][k]
        assert p.shape == (H, W, 3) and c.shape == depth.shape == conf.shape == (H, W) and normal.shape == (H, W, 3)
        assert p.dtype == c.dtype == np.float64 and depth.dtype == conf.dtype == normal.dtype == np.float32
        assert p.tobytes() == rp.tobytes(), f"state {k}: {int((p != rp).any(-1).sum())} planes differ"
        finite = np.isfinite(rc)
        assert np.array_equal(np.isfinite(c), finite) and np.isposinf(c[~finite]).all()
        worst = max(worst, float(np.abs(c[finite] - rc[finite]).max(initial=0.0)))
        assert np.abs(c[finite] - rc[finite]).max(initial=0.0) <= tol
        assert np.abs(conf.astype(np.float64) - rconf.astype(np.float64)).max() <= tol
        assert depth.tobytes() == rd.tobytes() and normal.tobytes() == rn.tobytes()
    check(0)
    k = 0
    for it in range(case["iterations"]):
        for colour in (0, 1):
            _step(case, dev, plane, cost, it, colour)
            k += 1
            check(k)
    assert k + 1 == len(ref["states"])
    print(f"\n{name}: {k} half-iterations, max |delta cost| {worst:.3e} (tolerance {tol:.3e}), "
          f"{int((ref['outs'][-1][0] > 0).sum())} of {H * W} pixels with depth")
    if name in ("facing_away", "constant_reference"):
        assert np.isposinf(cost.cpu().numpy()).all()
    # the whole call gives the state of the last step
    out = _refine(case)
    assert out.plane.cpu().numpy().tobytes() == ref["states"][-1][0].tobytes()
    assert out.depth.cpu().numpy().tobytes() == ref["outs"][-1][0].tobytes()
    assert out.normal.cpu().numpy().tobytes() == ref["outs"][-1][2].tobytes()


@pytest.mark.parametrize("name", P.TRUTH_CASES)
def test_kernel_against_truth(name):
    """The kernels from the GPU's own sweep under the bounds of tests/test_patchmatch_host.py::test_restatement_against_truth,
    and the three conditions against that sweep (the parent's result on the same case)."""
    case = P.cases()[name]
    dev = _device(case)
    sweep = mvs.plane_sweep(dev["frames"], dev["poses"], dev["cams"], case["ref"], case["sources"], case["depth_near"],
                            case["depth_far"], case["num_planes"], case["radius"], case["min_views"], case["min_variance"],
                            case["min_conf"], rays=dev["rays"])
    out = PM.refine_depth(dev["frames"], dev["poses"], dev["cams"], case["ref"], case["sources"], case["depth_near"],
                          case["depth_far"], iterations=case["iterations"], radius=case["radius"], min_views=case["min_views"],
                          min_variance=case["min_variance"], min_conf=case["min_conf"], seed=case["seed"], rays=dev["rays"],
                          num_planes=case["num_planes"])
    truth = P.truth_of(name)
    dw = (case["inv_depth_near"] - case["inv_depth_far"]) / float(case["num_planes"] - 1)
    s_med, s_p90, s_valid = P.truth_errors(sweep.depth.cpu().numpy(), truth, dw)
    depth, normal = out.depth.cpu().numpy(), out.normal.cpu().numpy()
    med, p90, valid = P.truth_errors(depth, truth, dw)
    angle = float(np.median(P.normal_angles(normal, depth > 0)))
    print(f"\n{name}: sweep median {s_med:.4f}, 90th percentile {s_p90:.4f}, valid {s_valid:.4f}; refined {med:.4f}, {p90:.4f}, "
          f"{valid:.4f}; median normal angle {angle:.3f} degrees")
    m_med, m_p90, m_angle = P.TRUTH_MEASURED[name]
    assert med <= 2 * m_med and p90 <= 2 * m_p90 and angle <= 2 * m_angle
    view = int(name[-1])
    assert med <= (0.5 * s_med if view in (0, 1) else s_med)
    assert valid >= s_valid
    lengths = np.linalg.norm(normal[depth > 0].astype(np.float64), axis=-1)
    assert np.abs(lengths - 1.0).max() < 1e-6 and (normal[depth == 0] == 0).all()


def test_refinement_is_deterministic_and_keeps_no_state():
    """The same call twice gives identical bits, and again after a call on other data; another seed gives other planes;
    iterations = 0 returns the start."""
    case, other = P.cases()["holes"], P.cases()["k08_21x35"]
    first = [t.cpu().numpy() for t in _refine(case)]
    second = [t.cpu().numpy() for t in _refine(case)]
    _refine(other)
    third = [t.cpu().numpy() for t in _refine(case)]
    for a, b, c in zip(first, second, third):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    reseeded = _refine(case, seed=case["seed"] + 1)
    assert reseeded.plane.cpu().numpy().tobytes() != first[3].tobytes()
    zero = _refine(case, iterations=0)
    ref = P.reference("holes")
    assert zero.plane.cpu().numpy().tobytes() == ref["states"][0][0].tobytes()
    assert zero.depth.cpu().numpy().tobytes() == ref["outs"][0][0].tobytes()


def test_refined_normals_go_into_the_fusion():
    """Refined.normal of the three views, stacked, is what fusion.fuse_depth_maps(normals=...) takes: it runs, and the
    fused normals stay within the per-view bound of the true plane's."""
    sc = P.scenes()[0.08]
    frames, poses, cams, rays = D(sc["frames"]), D(sc["poses"]), D(sc["cams"]), D(sc["rays"])
    sources = [[s for s in range(3) if s != v] for v in range(3)]
    outs = [PM.refine_depth(frames, poses, cams, v, sources[v], C.NEAR, C.FAR, min_variance=1e-5, rays=rays[0], num_planes=24)
            for v in range(3)]
    depth, normals = torch.stack([o.depth for o in outs]), torch.stack([o.normal for o in outs])
    assert normals.shape == (3, 24, 32, 3) and normals.dtype == torch.float32
    given = fusion.fuse_depth_maps(depth, poses, cams, sources, normals=normals, rays=rays, ray_index=sc["ray_index"])
    auto = fusion.fuse_depth_maps(depth, poses, cams, sources, rays=rays, ray_index=sc["ray_index"])
    towards = -C._plane()[3]
    angle = lambda cloud: float(np.median(np.degrees(np.arccos(np.clip(cloud.normal.cpu().numpy().astype(np.float64) @ towards, -1, 1)))))
    print(f"\nfused with the refined normals: {len(given.xyz)} points, median normal angle {angle(given):.3f} degrees; "
          f"with the fusion's own from the same maps: {len(auto.xyz)} points, {angle(auto):.3f} degrees")
    assert len(given.xyz) > 0 and np.isfinite(given.normal.cpu().numpy()).all()
    assert np.abs(np.linalg.norm(given.normal.cpu().numpy(), axis=-1) - 1.0).max() < 1e-5
    # a fused normal is the normalised sum of its views' normals, so it is no further from the truth than the worst of
    # them: the per-view bound of test_kernel_against_truth (2 x the largest measured median) holds for the cloud
    assert angle(given) <= 2 * max(m[2] for n, m in P.TRUTH_MEASURED.items() if "k08" in n)


def test_python_surface_defaults_and_refusals():
    """refine_depth from its own sweep and ray map; the thin public plane_cost; what the entries refuse raises."""
    case = P.cases()["k0_24x32"]
    dev = _device(case)
    out = PM.refine_depth(dev["frames"], dev["poses"], dev["cams"], case["ref"], case["sources"], case["depth_near"],
                          case["depth_far"], min_variance=case["min_variance"], num_planes=24)
    assert isinstance(out, PM.Refined) and out._fields == ("depth", "conf", "normal", "plane", "cost")
    assert out.depth.shape == (24, 32) and out.normal.shape == (24, 32, 3) and out.plane.dtype == torch.float64
    explicit = PM.refine_depth(dev["frames"], dev["poses"], dev["cams"], case["ref"], case["sources"], case["depth_near"],
                               case["depth_far"], min_variance=case["min_variance"], num_planes=24,
                               rays=mvs.pixel_rays(case["cams"][case["ref"]], 24, 32), depth_step=case["depth_step"])
    for a, b in zip(out, explicit):                                              # the defaults: the camera's ray map, two spacings
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    again = PM.plane_cost(dev["frames"], dev["poses"], dev["cams"], case["ref"], case["sources"], out.plane, min_variance=case["min_variance"])
    assert again.cpu().numpy().tobytes() == out.cost.cpu().numpy().tobytes()      # the stored cost is the stored plane's
    invalid = "invalid argument"
    for over in (dict(radius=0), dict(radius=4), dict(sources=[]), dict(sources=list(range(9))), dict(min_views=0), dict(min_views=3),
                 dict(ref=3), dict(ref=-1), dict(sources=[0, 3]), dict(sources=[0, 1]), dict(depth_near=5.0, depth_far=3.2),
                 dict(depth_step=-1.0), dict(depth_step=float("nan")), dict(slope_step=-0.5)):
        with pytest.raises(RuntimeError, match=invalid):
            _refine(case, **over)
    plane, cost = _start(case, dev)
    for it, colour in ((-1, 0), (0, 2), (0, -1)):
        with pytest.raises(RuntimeError, match=invalid):
            _step(case, dev, plane, cost, it, colour)
    for over in (dict(depth_near=0.0), dict(depth_far=float("inf")), dict(max_tilt_deg=91.0), dict(max_tilt_deg=-1.0), dict(iterations=-1),
                 dict(rays=case["rays"][:-1]), dict(init_depth=case["init_depth"][:-1]), dict(seed=-1)):
        with pytest.raises(ValueError):
            _refine(case, **over)
    with pytest.raises(RuntimeError, match="no CPU path"):
        PM.refine_depth(torch.from_numpy(case["frames"]), dev["poses"], dev["cams"], 1, [0, 2], 3.2, 5.0)
