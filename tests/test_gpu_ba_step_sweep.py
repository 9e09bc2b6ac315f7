"""The candidate evaluation of an LM iteration after its rewrite: point_step's sweep in directional form (fy = F dy and
E^T fy without the Jacobian blocks), the cameras' share of the model cost change taken from U | g in cam_update's body, and
that body run in point_step's prologue instead of as a launch of its own.

Reference: the CPU port (oracle/ba.py, solve_csr) from the same start on the compiled problem's own arrays, termination
tests off, 3 iterations.  Compared per iteration: cost, cost_change, relative_decrease (= cost change / model cost change,
the quantity the rewrite derives anew), step_norm, radius, the accept pattern; then the final cameras and points.

Tolerances.  tests/test_gpu_ba.py compares the same solver with the same port: cost 1e-9 (relative), radius 1e-5, accept
pattern equal, final rotation / translation 5e-6, points 5e-5, focal 1e-6 (relative), distortion 1e-7 -- taken over as they
are.  It has no bound for the three other fields, so theirs follow from those:
  cost_change         the difference of two costs, each within 1e-9 of itself: 2e-9 x cost (absolute);
  relative_decrease   cost_change / model change: the bound of cost_change over the model change, + 1e-9 (relative) for the
                      model change, which is a sum over the observations like the cost;
  step_norm           the solution of the damped reduced system: 1e-6 (relative) -- rounding 1e-16 x the condition of the
                      system, at most ~1e8 with the diagonal damped by 1 / radius = 1e-4 of itself, x 100.

What the PARENT library (3b409a2: full Jacobians, model cost change summed observation by observation) uses of these bounds
on the cases below, and what this tree uses -- worst case over all of them, as a fraction of the bound, measured on an MI355X
(PARENT_USED / CHANGE_USED below; profiles/r09_port_deviation_{parent,change}.txt have every case): both stay below 1.3e-4 of
every bound, and the rewrite moves no field by more than the two libraries differ from the port anyway (cost 1.23e-4 -> 1.19e-4,
model change 2.87e-5 -> 2.78e-5, step norm 2.5e-5 -> 1.1e-5 of their bounds).  The bounds are the existing file's, which
allows for 50-iteration solves of large scenes; at three iterations of 48 points the solver sits five orders below them.

Cases: 6 cameras x 48 points with tracks of 2 .. 6 views, for every block shape (SIMPLE_PINHOLE / SIMPLE_RADIAL, shared /
per-camera intrinsics, KD 0, 1, 2 and the only-k layout), the trivial, Huber and Cauchy loss, camera 0 constant, t_x of camera
1 constant, one constant point, constant intrinsics (one camera's, or the shared block).  A track cannot be longer than the
number of cameras, so the track lengths {2, 7, 8, 9, 17, 33} -- 8- and 16-lane groups with a partial last sweep, more
observations per lane than the 2 or 4 prefetched ones -- come with 34 cameras x 48 points.  Both run with the points in
ascending track length and shuffled, at 8 and 16 lanes per point, with and without the long-track variant (vgg_ba_tuning).
440 cameras x 60 points with per-camera intrinsics: the camera table (20 doubles per camera) exceeds 64 KB, point_step reads
the cameras from global memory and cam_update is a launch of its own.

The device counts the point_step launches that ran cam_update's body in their prologue (control block), so a silent
fall-back to the separate launch -- or a prologue that runs where it must not -- fails."""
import numpy as np
import pytest
import torch

import oracle.ba as OB
from tests.test_gpu_ba_glue import CTL_MERGED_STEP_SUMS, ctl_int
from tests.test_gpu_dist import _LockStep
from vggsfm_amd import _lib
from vggsfm_amd import ba as BA
from vggsfm_amd.ba_options import LOSS_ID, BundleAdjustmentOptions
from vggsfm_amd.dist import ShardedBA, shard_slice
from vggsfm_amd.scene import make_scene, perturb_for_ba

pytestmark = pytest.mark.gpu

CTL_FUSED_STEP_PROLOGUES = 144      # byte offset in the workspace: the int32 behind CTL_MERGED_STEP_SUMS
ITERATIONS = 3

TOL = dict(cost=1e-9, radius=1e-5, cost_change=2e-9, model_change=1e-9, step_norm=1e-6, rotation=5e-6, translation=5e-6,
           points=5e-5, focal=1e-6, extra=1e-7)

# worst fraction of each bound used over every case of this file, MI355X
PARENT_USED = dict(cost=1.23e-4, radius=6.6e-6, cost_change=5.5e-5, model_change=2.87e-5, step_norm=2.5e-5, rotation=2.1e-9,
                   translation=1.7e-7, points=1.4e-8, focal=1.6e-7, extra=1.03e-5)
CHANGE_USED = dict(cost=1.19e-4, radius=1.2e-5, cost_change=5.4e-5, model_change=2.78e-5, step_norm=1.1e-5, rotation=2.2e-9,
                   translation=1.4e-7, points=1.2e-8, focal=1.6e-7, extra=1.0e-5)

# (camera model, shared, refine focal, refine extra, constant intrinsics)
SHAPES = {
    "pinhole_shared_kd1": ("SIMPLE_PINHOLE", True, True, True, False),
    "pinhole_percam_kd1": ("SIMPLE_PINHOLE", False, True, True, True),
    "radial_shared_kd2": ("SIMPLE_RADIAL", True, True, True, False),
    "radial_percam_kd2": ("SIMPLE_RADIAL", False, True, True, True),
    "radial_shared_kd0": ("SIMPLE_RADIAL", True, False, False, False),
    "radial_percam_only_k": ("SIMPLE_RADIAL", False, False, True, True),
    "radial_shared_kd2_const_intr": ("SIMPLE_RADIAL", True, True, True, True),
}
LOSSES = {"TRIVIAL": 1.0, "HUBER": 1.0, "CAUCHY": 2.0}
LAUNCHES = [(8, 0), (8, 1), (16, 0), (16, 1)]       # (lanes per point, long-track variant)


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def track_scene(S, lengths, cam, shared, seed, shuffled):
    """make_scene's cameras, points and measurements; point p is seen by lengths[p] random frames.  The points come in
    ascending track length or shuffled."""
    lengths = np.asarray(lengths)
    N = len(lengths)
    sc = make_scene(S, N, cam, shared_camera=shared, seed=seed, full_visibility=True, outlier_frac=0.1)
    rng = np.random.Generator(np.random.PCG64(seed + 31))
    order = rng.permutation(N) if shuffled else np.argsort(lengths, kind="stable")
    mask = np.zeros((S, N), bool)
    for p, L in zip(range(N), lengths[order]):
        mask[rng.permutation(S)[:L], p] = True
    assert mask.sum(1).min() >= 2, "every camera sees something"
    return sc, mask, lengths[order]


def options(loss="TRIVIAL", scale=1.0, rf=True, rk=True, iters=ITERATIONS):
    opt = BundleAdjustmentOptions()
    so = opt.solver_options
    so.max_num_iterations = iters
    so.function_tolerance = so.gradient_tolerance = so.parameter_tolerance = 0.0
    opt.refine_focal_length, opt.refine_extra_params = rf, rk
    opt.loss_function_type, opt.loss_function_scale = loss, scale
    return opt


def compile_case(sc, mask, cam, shared, rf, rk, const_intr, seed, sort_points):
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=seed)
    prob, _, deleted = BA.compile_problem(D(pts0), D(ext0), D(K0), D(sc.tracks), D(mask), D(extra0), shared, cam,
                                          refine_focal_length=rf, refine_extra_params=rk, sort_points=sort_points)
    assert not bool(deleted.any())
    C, P, NI = prob.cam_t.shape[0], prob.pts.shape[0], prob.intr.shape[0]
    # the default gauge: camera 0 constant, t_x of camera 1 constant; + one constant point, + constant intrinsics
    assert prob.cam_const.cpu().tolist()[:2] == [1, 2]
    pc = torch.zeros(P, dtype=torch.uint8, device="cuda")
    pc[P // 3] = 1
    prob.pt_const = pc
    if const_intr:
        ic = torch.zeros(NI, dtype=torch.uint8, device="cuda")
        ic[min(2, NI - 1)] = 1
        prob.intr_const = ic
    return prob


def port_solve(prob, opt):
    """oracle/ba.py on the compiled problem's arrays (copies): (summary, cam_q, cam_t, intr, pts)"""
    h = lambda t, dt: None if t is None else np.ascontiguousarray(t.detach().cpu().numpy().astype(dt))
    C, NI = prob.cam_t.shape[0], prob.intr.shape[0]
    q, t, intr, pts = h(prob.cam_q, np.float64), h(prob.cam_t, np.float64), h(prob.intr, np.float64), h(prob.pts, np.float64)
    cam_intr = np.zeros(C, np.int32) if NI == 1 else np.arange(C, dtype=np.int32)
    so = opt.solver_options
    summ = OB.solve_csr(q, t, intr, pts, cam_intr, h(prob.row_ptr, np.int32), h(prob.obs_cam, np.int32),
                        h(prob.obs_uv, np.float64), prob.camera_model,
                        OB.ceres_options(so.max_num_iterations, 0.0, 0.0, 0.0), refine_focal=opt.refine_focal_length,
                        refine_extra=opt.refine_extra_params, loss=LOSS_ID[opt.loss_function_type],
                        loss_scale=opt.loss_function_scale, cam_const=h(prob.cam_const, np.uint8),
                        intr_const=h(prob.intr_const, np.uint8), pt_const=h(prob.pt_const, np.uint8))
    return summ, q, t, intr, pts


def used_fractions(sg, so, got, ref):
    """{field: worst |difference| / bound} of a GPU solve (summary sg, final state got) against the port's (so, ref); the
    accept pattern must be equal outright."""
    used = {k: 0.0 for k in TOL}
    assert len(sg["iterations"]) == len(so["iterations"]) == ITERATIONS + 1
    for a, b in zip(sg["iterations"], so["iterations"]):
        assert a["iteration"] == b["iteration"] and a["successful"] == b["successful"], (a, b)
        cost = b["cost"]
        used["cost"] = max(used["cost"], abs(a["cost"] - cost) / (TOL["cost"] * cost))
        used["radius"] = max(used["radius"], abs(a["radius"] - b["radius"]) / (TOL["radius"] * b["radius"]))
        if b["iteration"] == 0:
            continue
        # (the trajectory stays above the floor where the step quality is rounding noise in both implementations)
        assert abs(b["cost_change"]) > 1e-6 * cost, b
        prev = cost + b["cost_change"] if b["successful"] else cost
        cc_bound = TOL["cost_change"] * prev
        used["cost_change"] = max(used["cost_change"], abs(a["cost_change"] - b["cost_change"]) / cc_bound)
        rel_bound = abs(b["relative_decrease"]) * (cc_bound / abs(b["cost_change"]) + TOL["model_change"])
        used["model_change"] = max(used["model_change"], abs(a["relative_decrease"] - b["relative_decrease"]) / rel_bound)
        used["step_norm"] = max(used["step_norm"], abs(a["step_norm"] - b["step_norm"]) / (TOL["step_norm"] * b["step_norm"]))
    q, t, intr, pts = (x.cpu().numpy() for x in got)
    rq, rt, rintr, rpts = ref
    used["rotation"] = np.abs(q - rq).max() / TOL["rotation"]
    used["translation"] = np.abs(t - rt).max() / TOL["translation"]
    used["points"] = np.abs(pts - rpts).max() / TOL["points"]
    used["focal"] = (np.abs(intr[:, 0] - rintr[:, 0]) / rintr[:, 0]).max() / TOL["focal"]
    used["extra"] = np.abs(intr[:, 3] - rintr[:, 3]).max() / TOL["extra"]
    return {k: float(v) for k, v in used.items()}


_PORT = {}      # the port's solve of a case, computed once


def deviations(key, build, opt, launches):
    """Solves the case built by `build(sort_points)` on the GPU with every launch variant, points ascending and shuffled,
    against the port: ({field: worst fraction of its bound}, [fused prologue count of every solve], [iterations])."""
    L = _lib.lib()
    worst, fused, iters = {k: 0.0 for k in TOL}, [], []
    try:
        for shuffled in (False, True):
            for lpp, longt in launches:
                prob = build(shuffled)
                if (key, shuffled) not in _PORT:
                    _PORT[(key, shuffled)] = port_solve(prob, opt)
                so, *ref = _PORT[(key, shuffled)]
                assert L.vgg_ba_tuning(lpp, longt, 0, 0) == 0
                sg, ws = BA.solve(prob, opt)
                used = used_fractions(sg, so, (prob.cam_q, prob.cam_t, prob.intr, prob.pts), ref)
                worst = {k: max(worst[k], used[k]) for k in TOL}
                fused.append(ctl_int(ws, CTL_FUSED_STEP_PROLOGUES))
                iters.append((sg["num_iterations"], ctl_int(ws, CTL_MERGED_STEP_SUMS)))
    finally:
        L.vgg_ba_tuning(0, -1, 0, 0)
    return worst, fused, iters


def small_case(shape, loss):
    cam, shared, rf, rk, const_intr = SHAPES[shape]
    lengths = np.resize(np.array([2, 3, 4, 5, 6, 6]), 48)
    opt = options(loss, LOSSES[loss], rf, rk)

    def build(shuffled):
        sc, mask, _ = track_scene(6, lengths, cam, shared, 41, shuffled)
        return compile_case(sc, mask, cam, shared, rf, rk, const_intr, 41, sort_points=not shuffled)
    return (shape, loss), build, opt


def long_track_case(shape):
    cam, shared, rf, rk, const_intr = SHAPES[shape]
    lengths = np.resize(np.array([2, 7, 8, 9, 17, 33]), 48)
    opt = options("TRIVIAL", 1.0, rf, rk)

    def build(shuffled):
        sc, mask, got = track_scene(34, lengths, cam, shared, 43, shuffled)
        prob = compile_case(sc, mask, cam, shared, rf, rk, const_intr, 43, sort_points=not shuffled)
        counts = np.diff(prob.row_ptr.cpu().numpy())
        assert sorted(set(counts.tolist())) == [2, 7, 8, 9, 17, 33]
        assert (np.diff(counts) >= 0).all() != shuffled
        return prob
    return ("long", shape), build, opt


def check(worst, fused, iters, expect_fused):
    print("fraction of the bound used:", {k: f"{v:.3g}" for k, v in worst.items()}, "prologues", fused)
    for (n, sums), f in zip(iters, fused):
        assert n == sums == ITERATIONS                      # (every iteration reached the step)
        assert f == (ITERATIONS if expect_fused else 0), (f, n)
    for k, v in worst.items():
        assert v <= 1.0, (k, v, TOL[k])


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_six_cameras_match_the_port(shape, loss):
    check(*deviations(*small_case(shape, loss), LAUNCHES), expect_fused=True)


@pytest.mark.parametrize("shape", ["radial_shared_kd2", "radial_percam_kd2", "pinhole_shared_kd1"])
def test_track_lengths_across_the_lane_groups_match_the_port(shape):
    check(*deviations(*long_track_case(shape), LAUNCHES), expect_fused=True)


def big_table_case():
    cam, shared = "SIMPLE_RADIAL", False
    lengths = np.full(60, 150)
    opt = options()

    def build(shuffled):
        sc, mask, _ = track_scene(440, lengths, cam, shared, 47, shuffled)
        return compile_case(sc, mask, cam, shared, True, True, True, 47, sort_points=not shuffled)
    return ("big",), build, opt


def test_camera_table_over_64_kb_keeps_the_cam_update_launch():
    """20 doubles per camera x 440 cameras = 70400 bytes: no LDS table, so no prologue -- the count is zero."""
    check(*deviations(*big_table_case(), [(0, -1)]), expect_fused=False)


@pytest.mark.parametrize("in_place", [False, True])
def test_two_ranks_in_lock_step_match_one_rank(in_place):
    """tests/test_gpu_dist.py's emulation and bounds, both exchange forms, on 6 cameras x 48 points.  U | g are all-reduced
    and every rank adds the cameras' share of the model cost change un-reduced: counted once per rank, or not at all, the
    step quality -- and with it the radius and every later cost -- leaves the single-rank trajectory."""
    cam, shared, world, iters = "SIMPLE_RADIAL", True, 2, 6
    lengths = np.resize(np.array([2, 3, 4, 5, 6, 6]), 48)
    sc, mask, _ = track_scene(6, lengths, cam, shared, 41, True)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=41)
    opts = options(iters=iters)
    prob, _, _ = BA.compile_problem(D(pts0), D(ext0), D(K0), D(sc.tracks), D(mask), D(extra0), shared, cam)
    ref = ShardedBA(prob, opts).solve()
    solvers, problems = [], []
    for r in range(world):
        tr, mk, pt, _ = shard_slice(D(sc.tracks), D(mask), D(pts0), r, world)
        pr, _, _ = BA.compile_problem(pt, D(ext0), D(K0), tr, mk, D(extra0), shared, cam)
        problems.append(pr)
        solvers.append(ShardedBA(pr, opts, rank=r, world_size=world, all_reduce=lambda t, op: None))
    hub = _LockStep(world)
    for s in solvers:
        s.begin()
    for _ in range(iters + 1):
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
    for s in solvers:
        o = s.finish(20)
        assert o["num_iterations"] == ref["num_iterations"] == iters and o["termination"] == ref["termination"]
        assert abs(o["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]
        for a, b in zip(o["iterations"], ref["iterations"]):
            assert a["successful"] == b["successful"] and abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"], (a, b)
            if b["iteration"] > 0:
                # (relative_decrease from costs within 1e-9: the bound of used_fractions)
                prev = b["cost"] + b["cost_change"] if b["successful"] else b["cost"]
                bound = abs(b["relative_decrease"]) * (2e-9 * prev / abs(b["cost_change"]) + 1e-9)
                assert abs(a["relative_decrease"] - b["relative_decrease"]) <= bound, (a, b)
        assert ctl_int(s.ws, CTL_FUSED_STEP_PROLOGUES) == iters
    for pr in problems:
        np.testing.assert_allclose(pr.cam_q.cpu().numpy(), prob.cam_q.cpu().numpy(), atol=1e-9)
        np.testing.assert_allclose(pr.cam_t.cpu().numpy(), prob.cam_t.cpu().numpy(), atol=1e-9)
        np.testing.assert_allclose(pr.intr.cpu().numpy(), prob.intr.cpu().numpy(), rtol=1e-10)
    got = torch.cat([pr.pts for pr in problems]).cpu().numpy()
    np.testing.assert_allclose(got, prob.pts.cpu().numpy(), atol=1e-8)
