"""The linearisation at the candidate (cam_pass<CAND>, phase 2): its cost decides the step, and on acceptance its U_c, g_c,
cost become reduce buffer 0 without a pass at the start of the next iteration.  Checked on solves with rejected steps
(min_relative_decrease 0.9 rejects about half of the steps of these scenes): the oracle's trajectory, the buffer against a
fresh start-point pass at the same x, and two ranks in lock step against one."""
import numpy as np
import pytest
import torch

from oracle import ba as OB
from tests.test_gpu_ba import _compare_trajectories
from tests.test_gpu_dist import _LockStep
from vggsfm_amd import ba as BA
from vggsfm_amd.dist import ShardedBA, shard_slice
from vggsfm_amd.scene import make_scene, perturb_for_ba
from vggsfm_amd.utils.triangulation_helpers import prepare_ba_options

pytestmark = pytest.mark.gpu

CASES = [("SIMPLE_RADIAL", True), ("SIMPLE_PINHOLE", False), ("SIMPLE_RADIAL", False)]
MIN_REL_DECREASE = 0.9       # (oracle, 24 x 1500, seed 17, 12 iterations: 5 or 6 of the 12 steps rejected)


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _scene(cam, shared):
    sc = make_scene(24, 1500, cam, shared_camera=shared, seed=17)
    return sc, perturb_for_ba(sc, seed=17)


def _gpu_opts(iters=12):
    o = prepare_ba_options()
    o.solver_options.max_num_iterations = iters
    o.solver_options.min_relative_decrease = MIN_REL_DECREASE
    return o


@pytest.mark.parametrize("cam,shared", CASES)
def test_rejected_steps_follow_the_oracle_trajectory(cam, shared):
    sc, (ext0, K0, extra0, pts0) = _scene(cam, shared)
    oo = OB.prepare_ba_options()
    oo.max_num_iterations = 12
    oo.min_relative_decrease = MIN_REL_DECREASE
    po, eo, Ko, xo, so = OB.bundle_adjustment(pts0, ext0, K0, sc.tracks, sc.mask, extra0, shared, cam, oo)
    assert so["num_unsuccessful_steps"] >= 3
    pts, ext, K, extra, sg = BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0),
                                                  shared, cam, _gpu_opts())
    assert sg["num_unsuccessful_steps"] == so["num_unsuccessful_steps"]
    assert abs(sg["initial_cost"] - so["initial_cost"]) <= 1e-11 * so["initial_cost"]
    _compare_trajectories(sg, so, 12)
    assert abs(sg["final_cost"] - so["final_cost"]) <= 1e-8 * so["final_cost"]
    np.testing.assert_allclose(ext.cpu().numpy(), eo, rtol=0, atol=5e-6)
    np.testing.assert_allclose(pts.cpu().numpy(), po, rtol=0, atol=5e-5)


@pytest.mark.parametrize("cam,shared", CASES)
def test_buffer_0_equals_a_fresh_pass_after_every_step(cam, shared):
    """After every iteration -- accepted (buffer 0 = the candidate's terms) or rejected (buffer 0 kept) -- reduce buffer 0
    is bit for bit what the start-point pass of a new solve at the same parameters computes."""
    sc, (ext0, K0, extra0, pts0) = _scene(cam, shared)
    prob, _, _ = BA.compile_problem(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), D(extra0), shared, cam)
    opts = _gpu_opts()
    s = ShardedBA(prob, opts)
    s.begin()
    seen = set()
    for it in range(8):
        s.iteration()
        log = s.finish(it + 2)["iterations"]
        seen.add(bool(log[it + 1]["successful"]))
        fresh = ShardedBA(prob, opts)
        fresh.begin()
        torch.cuda.synchronize()
        a, b = s.bufs[0].cpu().numpy(), fresh.bufs[0].cpu().numpy()
        assert np.isfinite(a).all()
        assert np.array_equal(a, b), (it, np.abs(a - b).max())
    assert seen == {True, False}


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("cam,shared", CASES[:2])
def test_two_ranks_with_rejected_steps_equal_one(cam, shared, in_place):
    """Two ranks in lock step (collectives emulated on the solvers' own reduce buffers, as in tests/test_gpu_dist.py): the
    candidate's cost travels in buffer 3, its camera-side terms in buffer 0 of the next iteration, and after a rejected
    step the SUM of buffer 0 gives back the kept terms."""
    sc, (ext0, K0, extra0, pts0) = _scene(cam, shared)
    opts = _gpu_opts()
    prob, _, _ = BA.compile_problem(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), D(extra0), shared, cam)
    ref = ShardedBA(prob, opts).solve()
    assert ref["num_unsuccessful_steps"] >= 3
    world = 2
    solvers, problems = [], []
    for r in range(world):
        tr, mk, pt, _ = shard_slice(D(sc.tracks), D(sc.mask), D(pts0), r, world)
        pr, _, _ = BA.compile_problem(pt, D(ext0), D(K0), tr, mk, D(extra0), shared, cam)
        problems.append(pr)
        solvers.append(ShardedBA(pr, opts, rank=r, world_size=world, all_reduce=lambda t, op: None, split_exchange=False))
    hub = _LockStep(world)
    for s in solvers:
        s.begin()
    for _ in range(opts.solver_options.max_num_iterations + 1):
        for s in solvers:
            s._phase(0)
        hub.exchange([s.bufs[0] for s in solvers], "sum")
        for s in solvers:
            s._phase(1)
            s._phase(4)
        if in_place:
            chunk = -(-solvers[0].bufs[4].numel() // world)
            total = torch.stack([s._padded for s in solvers]).sum(0)
            for r, s in enumerate(solvers):
                s._mine[:chunk].copy_(total[r * chunk:(r + 1) * chunk])
            allm = torch.cat([s._mine for s in solvers])
            for s in solvers:
                s._gathered.copy_(allm)
                s._phase(6)
        else:
            hub.exchange([s.bufs[4] for s in solvers], "sum")
            for s in solvers:
                s._phase(5)
            hub.exchange([s.bufs[2] for s in solvers], "max")
        for s in solvers:
            s._phase(2)
        hub.exchange([s.bufs[3] for s in solvers], "sum")
        for s in solvers:
            s._phase(3)
    for o in (s.finish(20) for s in solvers):
        assert o["num_iterations"] == ref["num_iterations"] and o["termination"] == ref["termination"]
        assert o["num_unsuccessful_steps"] == ref["num_unsuccessful_steps"]
        assert abs(o["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]
        for a, b in zip(o["iterations"], ref["iterations"]):
            assert a["successful"] == b["successful"] and abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"]
    for pr in problems:
        np.testing.assert_allclose(pr.cam_q.cpu().numpy(), prob.cam_q.cpu().numpy(), atol=1e-9)
        np.testing.assert_allclose(pr.cam_t.cpu().numpy(), prob.cam_t.cpu().numpy(), atol=1e-9)
        np.testing.assert_allclose(pr.intr.cpu().numpy(), prob.intr.cpu().numpy(), rtol=1e-10)
    got = torch.cat([pr.pts for pr in problems]).cpu().numpy()
    np.testing.assert_allclose(got, prob.pts.cpu().numpy(), atol=1e-8)
