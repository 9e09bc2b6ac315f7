"""The serial glue of an LM iteration in fewer launches: tile sums + assembly + preparation in one kernel
(tile_assemble_kernel), the step sums in the last workgroup of cam_reduce.  Both compute the same sums in the same order as
the separate launches they replace, which stay in the library behind vgg_ba_set_tile_rhs(2 | 4): every case solves a few LM
iterations on both paths and compares the iteration logs and the results bit for bit."""
import numpy as np
import pytest
import torch

from vggsfm_amd import _lib
from vggsfm_amd import ba as BA
from vggsfm_amd.ba_options import BundleAdjustmentOptions
from vggsfm_amd.dist import ShardedBA, shard_slice
from vggsfm_amd.scene import make_scene, perturb_for_ba

pytestmark = pytest.mark.gpu

LEGACY_GLUE = 4            # bit 2 of vgg_ba_set_tile_rhs: the separate glue launches
# byte offsets in the workspace of three int32 of the solve's control block (ten doubles, then the int32 fields): the arrival
# counter of the step sums, and how often the solve ran tile_assemble_kernel / the step sums inside cam_reduce_kernel
CTL_STEP_ARRIVALS, CTL_MERGED_GLUE, CTL_MERGED_STEP_SUMS = 132, 136, 140


def ctl_int(ws, offset):
    return int(ws[offset:offset + 4].view(torch.int32).item())


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def window_scene(S, N, cam, shared, seed, lo=3, hi=12, masked_frames=None, outlier_frac=0.05):
    """make_scene's cameras, points and measurements with tracks of lo..hi consecutive views."""
    sc = make_scene(S, N, cam, shared_camera=shared, seed=seed, full_visibility=True, outlier_frac=outlier_frac)
    rng = np.random.Generator(np.random.PCG64(seed + 77))
    length = rng.integers(lo, hi + 1, size=N)
    start = (rng.uniform(0.0, 1.0, size=N) * (S - length + 1)).astype(np.int64)
    frames = np.arange(S)[:, None]
    mask = (frames >= start[None]) & (frames < (start + length)[None])
    if masked_frames is not None:
        mask[masked_frames[0]:masked_frames[1]] = False
    return sc, mask


def lm_options(iters, terminate=False):
    opt = BundleAdjustmentOptions()
    so = opt.solver_options
    so.max_num_iterations = iters
    if not terminate:
        so.function_tolerance = so.gradient_tolerance = so.parameter_tolerance = 0.0
    return opt


def groups_with_diagonal_tile(prob):
    td = prob.tile_desc.cpu().numpy()
    return set(int(g) for g in td[td[:, 0] == td[:, 1], 0])


def all_groups(prob):
    return set(range(-(-prob.cam_t.shape[0] // BA.GROUP)))


def solve_both(start, mask, sc, cam, shared, opt, expect_fused=True):
    """one solve on the merged launches, one on the separate ones; returns the two (outputs, summary)"""
    ext0, K0, extra0, pts0 = start
    L = _lib.lib()
    out = []
    try:
        for sel in (2, 2 | LEGACY_GLUE):
            assert L.vgg_ba_set_tile_rhs(sel) == 0
            prob, _, _ = BA.compile_problem(D(pts0), D(ext0), D(K0), D(sc.tracks), D(mask), D(extra0), shared, cam)
            # (what selects the launches: a camera group without a diagonal tile takes the separate ones)
            assert (groups_with_diagonal_tile(prob) == all_groups(prob)) == expect_fused
            summ, ws = BA.solve(prob, opt)
            # which kernels ran, from the device: the merged launch once per iteration that reached phase 1 (the last one only checks), the step sums in
            # cam_reduce once per iteration that reached phase 2 -- and neither behind the selector
            glue, sums = ctl_int(ws, CTL_MERGED_GLUE), ctl_int(ws, CTL_MERGED_STEP_SUMS)
            if sel & LEGACY_GLUE:
                assert glue == 0 and sums == 0
            else:
                assert sums == summ["num_iterations"] > 0 and (glue >= sums if expect_fused else glue == 0), (glue, sums)
            out.append((prob.cam_q, prob.cam_t, prob.intr, prob.pts, summ))
    finally:
        L.vgg_ba_set_tile_rhs(2)
    return out


def assert_same_bits(a, b):
    assert a[4]["num_iterations"] == b[4]["num_iterations"] and a[4]["termination"] == b[4]["termination"]
    assert len(a[4]["iterations"]) == len(b[4]["iterations"])
    for ia, ib in zip(a[4]["iterations"], b[4]["iterations"]):
        for key in ("cost", "radius", "successful", "gradient_max_norm", "step_norm", "cost_change", "relative_decrease"):
            assert ia[key] == ib[key], (key, ia, ib)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("merged", [True, False])
def test_shared_radial_partial_last_group(merged, monkeypatch):
    """33 frames: the third camera group holds ONE camera.  Default (COLMAP) gauge: pose 0 and t_x of camera 1 constant."""
    if not merged:
        monkeypatch.setattr(BA, "MERGED_TILE_MAX_OBS", 0)
    sc, mask = window_scene(33, 400, "SIMPLE_RADIAL", True, seed=5)
    a, b = solve_both(perturb_for_ba(sc, seed=5), mask, sc, "SIMPLE_RADIAL", True, lm_options(7))
    assert a[4]["num_iterations"] == 7
    assert_same_bits(a, b)
    np.testing.assert_array_equal(a[1][0].cpu().numpy(), sc.extrinsics[0, :, 3])    # the gauge frame stayed
    assert a[1][1, 0].item() == perturb_for_ba(sc, seed=5)[0][1, 0, 3]              # and t_x of camera 1


@pytest.mark.parametrize("merged", [True, False])
@pytest.mark.parametrize("cam", ["SIMPLE_PINHOLE", "SIMPLE_RADIAL"])
def test_per_frame_intrinsics(cam, merged, monkeypatch):
    """7 x 7 and 8 x 8 tile blocks (full Schur factors): the right-hand side's two entry pairs meet in one workgroup."""
    if not merged:
        monkeypatch.setattr(BA, "MERGED_TILE_MAX_OBS", 0)
    sc, mask = window_scene(20, 300, cam, False, seed=9)
    a, b = solve_both(perturb_for_ba(sc, seed=9), mask, sc, cam, False, lm_options(6))
    assert a[4]["num_iterations"] == 6
    assert_same_bits(a, b)


# perturb_for_ba arguments of the rejected-step case.  The CPU port (oracle/ba.py) from this start, seed 5: iterations 1, 2
# accepted, 3 .. 6 rejected (the radius shrinks four times), 7 and 8 accepted.
FAR_START = dict(rot_deg=4.0, trans=0.3, focal_rel=0.1, point=0.3)


def test_rejected_step_keeps_the_linearisation():
    """A start far from the optimum: at least one step is rejected (reduce buffer 0 stays, need_lin is not set, the merged
    launch runs no prep_body) and at least one accepted."""
    sc, mask = window_scene(33, 400, "SIMPLE_RADIAL", True, seed=5)
    a, b = solve_both(perturb_for_ba(sc, seed=5, **FAR_START), mask, sc, "SIMPLE_RADIAL", True, lm_options(8))
    flags = [it["successful"] for it in a[4]["iterations"][1:]]
    assert any(flags) and not all(flags), flags
    assert_same_bits(a, b)


def test_group_without_observations_takes_the_separate_launches():
    """frames 16..31 of 40 see nothing: the second camera group has no diagonal tile, nobody would add its cameras' terms in
    the merged launch -- the solve falls back to the separate ones, and solves."""
    sc, mask = window_scene(40, 400, "SIMPLE_RADIAL", True, seed=13, masked_frames=(16, 32))
    a, b = solve_both(perturb_for_ba(sc, seed=13), mask, sc, "SIMPLE_RADIAL", True, lm_options(6), expect_fused=False)
    assert_same_bits(a, b)
    assert a[4]["final_cost"] < 0.5 * a[4]["initial_cost"]
    assert all(bool(torch.isfinite(x).all()) for x in a[:4])


def test_two_ranks_in_lock_step_match_one_rank():
    """The first case on two ranks (tests/test_gpu_dist.py's emulation and tolerances): rank 1 adds no global terms, every
    rank keeps its own arrival counter."""
    cam, shared, world = "SIMPLE_RADIAL", True, 2
    sc, mask = window_scene(33, 400, cam, shared, seed=5)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=5)
    opts = lm_options(7)
    prob, _, _ = BA.compile_problem(D(pts0), D(ext0), D(K0), D(sc.tracks), D(mask), D(extra0), shared, cam)
    ref = ShardedBA(prob, opts).solve()
    solvers, problems = [], []
    for r in range(world):
        tr, mk, pt, _ = shard_slice(D(sc.tracks), D(mask), D(pts0), r, world)
        pr, _, _ = BA.compile_problem(pt, D(ext0), D(K0), tr, mk, D(extra0), shared, cam)
        assert groups_with_diagonal_tile(pr) == all_groups(pr)
        problems.append(pr)
        solvers.append(ShardedBA(pr, opts, rank=r, world_size=world, all_reduce=lambda t, op: None))

    def exchange(tensors, op):
        stacked = torch.stack(tensors)
        red = stacked.max(0).values if op == "max" else stacked.sum(0)
        for t in tensors:
            t.copy_(red)
    for s in solvers:
        s.begin()
    for _ in range(opts.solver_options.max_num_iterations + 1):
        for s in solvers:
            s._phase(0)
        exchange([s.bufs[0] for s in solvers], "sum")
        for s in solvers:
            s._phase(1)
            s._phase(4)
        exchange([s.bufs[4] for s in solvers], "sum")
        for s in solvers:
            s._phase(5)
        exchange([s.bufs[2] for s in solvers], "max")
        for s in solvers:
            s._phase(2)
        exchange([s.bufs[3] for s in solvers], "sum")
        for s in solvers:
            s._phase(3)
    for s in solvers:
        o = s.finish(20)
        assert o["num_iterations"] == ref["num_iterations"] and o["termination"] == ref["termination"]
        assert abs(o["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]
        for x, y in zip(o["iterations"], ref["iterations"]):
            assert x["successful"] == y["successful"] and abs(x["cost"] - y["cost"]) <= 1e-9 * y["cost"]
        assert ctl_int(s.ws, CTL_STEP_ARRIVALS) == 0
        assert ctl_int(s.ws, CTL_MERGED_GLUE) >= o["num_iterations"] == ctl_int(s.ws, CTL_MERGED_STEP_SUMS) > 0
    for pr in problems:
        np.testing.assert_allclose(pr.cam_q.cpu().numpy(), prob.cam_q.cpu().numpy(), atol=1e-9)
        np.testing.assert_allclose(pr.cam_t.cpu().numpy(), prob.cam_t.cpu().numpy(), atol=1e-9)
        np.testing.assert_allclose(pr.intr.cpu().numpy(), prob.intr.cpu().numpy(), rtol=1e-10)
    got = torch.cat([pr.pts for pr in problems]).cpu().numpy()
    np.testing.assert_allclose(got, prob.pts.cpu().numpy(), atol=1e-8)


def test_counter_is_zero_past_termination_and_workspace_is_reusable():
    """vgg_ba_solve enqueues iterations past the termination (no-ops): the arrival counter reads 0 afterwards, and a second
    solve in the same workspace gives the bits of the first.  (Without outliers: the CPU port meets the gradient tolerance in
    iteration 16 of this case; with them it is still descending after 50.)"""
    cam, shared = "SIMPLE_RADIAL", True
    sc, mask = window_scene(33, 400, cam, shared, seed=5, outlier_frac=0.0)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=5)
    opt = lm_options(30, terminate=True)
    ws, runs = None, []
    for _ in range(2):
        prob, _, _ = BA.compile_problem(D(pts0), D(ext0), D(K0), D(sc.tracks), D(mask), D(extra0), shared, cam)
        out, ws2 = BA.solve(prob, opt, ws)
        assert ws is None or ws2 is ws
        ws = ws2
        assert out["termination"] != 0 and out["num_iterations"] < 30, out["termination_str"]
        assert ctl_int(ws, CTL_STEP_ARRIVALS) == 0
        assert ctl_int(ws, CTL_MERGED_GLUE) > 0 and ctl_int(ws, CTL_MERGED_STEP_SUMS) == out["num_iterations"]
        runs.append((out, prob.cam_q.clone(), prob.cam_t.clone(), prob.intr.clone(), prob.pts.clone()))
    (o1, *t1), (o2, *t2) = runs
    assert [(i["cost"], i["radius"], i["successful"], i["gradient_max_norm"]) for i in o1["iterations"]] == \
           [(i["cost"], i["radius"], i["successful"], i["gradient_max_norm"]) for i in o2["iterations"]]
    for x, y in zip(t1, t2):
        assert torch.equal(x, y)
