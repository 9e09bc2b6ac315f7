"""The pose-refinement case table shared by tests/test_pose_cases.py (CPU: the oracle alone) and
tests/test_gpu_pose_regimes.py (GPU: ``vgg_pose_refine`` against the oracle).

A case is one frame of a synthetic scene (vggsfm_amd.scene) with a start pose, an inlier mask, refine flags, a
``vgg_ba_options`` setting, a loss and a track precision.  `build` makes the arrays, `solve` runs oracle/ba_oracle.c on
them through ``oracle.ba.pose_refinement``, `admission` evaluates -- from the oracle and nothing else -- whether the
reference is stable enough on the case to be a yardstick, and `run_kernel` is the raw ctypes driver of the device entry.

Only numpy and the oracle are needed to import this module; `run_kernel` imports torch and the library when called.
"""
import ctypes
import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import ba as OB
from vggsfm_amd.scene import make_scene, perturb_for_ba

S = 6
PERTURB = {"easy": dict(rot_deg=1.0, trans=0.05, focal_rel=0.02),       # the start of tests/test_gpu_pose.py
           "hard": dict(rot_deg=15.0, trans=0.5, focal_rel=0.3),
           "far": dict(rot_deg=30.0, trans=1.0, focal_rel=0.5)}
TERMINATION = {0: "cap", 1: "gradient", 2: "function", 3: "parameter", 4: "radius", 5: "failure"}
INT_KEYS = ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "termination", "n_reduced")
PINHOLE_INTR3 = 0.375          # what a SIMPLE_PINHOLE case keeps in the unused fourth intrinsic: it must come back untouched


@dataclass(frozen=True)
class Case:
    name: str
    model: str = "SIMPLE_RADIAL"
    flags: int = 3                 # bit 0 focal, bit 1 extra
    frame: int = 2
    pert: str = "easy"
    n: int = -1                    # >= 0: the first n non-outlier inliers only
    P: int = 800                   # != 800: a scene of P points, all of them inliers
    opt: tuple = ()                # ((field of vgg_ba_options, value), ...) over RefineAbsolutePose's options
    loss: int = 1                  # 0 trivial, 1 Cauchy, 2 Huber, 3 SoftL1
    scale: float = 1.0
    tracks: str = "f32"            # "f32" | "f64" (tracks that float32 cannot hold)
    tz: float = 0.0                # added to the start translation's z
    inf_obs: bool = False          # one inlier observation coordinate = +inf
    nan_pt: bool = False           # one inlier point coordinate = NaN
    twin: str = ""                 # option cases: the case with the same problem whose oracle solve must differ
    finite: bool = field(default=True, init=False)

    def __post_init__(self):
        object.__setattr__(self, "finite", not (self.inf_obs or self.nan_pt))


def _o(**kw):
    return tuple(sorted(kw.items()))


HARD5 = dict(pert="hard", frame=5)
CASES = [
    # --- the easy trajectory of tests/test_gpu_pose.py, every flag combination, and SIMPLE_PINHOLE with bit 1 set
    Case("easy_radial_fk"),
    Case("easy_radial_f", flags=1),
    Case("easy_radial_k", flags=2),
    Case("easy_radial_pose", flags=0),
    Case("easy_pinhole_f", model="SIMPLE_PINHOLE", flags=1),
    Case("easy_pinhole_pose", model="SIMPLE_PINHOLE", flags=0),
    Case("easy_pinhole_bit1", model="SIMPLE_PINHOLE", flags=3),
    Case("easy_pinhole_bit1_only", model="SIMPLE_PINHOLE", flags=2),
    # --- rejected steps
    Case("hard_pinhole_f", model="SIMPLE_PINHOLE", flags=1, **HARD5),
    Case("hard_pinhole_pose", model="SIMPLE_PINHOLE", flags=0, **HARD5),
    Case("hard_radial_fk", **HARD5),
    Case("hard_radial_f", flags=1, **HARD5),
    Case("hard_radial_pose", flags=0, **HARD5),
    Case("far_pinhole_f", model="SIMPLE_PINHOLE", flags=1, pert="far"),
    # (start translation pulled back along z: 685 / 381 / 514 of the frame's inliers start behind the camera)
    Case("behind_radial_pose_hard", flags=0, pert="hard", tz=-4.5),
    Case("behind_pinhole_pose_hard", model="SIMPLE_PINHOLE", flags=0, pert="hard", tz=-4.5),
    Case("behind_pinhole_pose", model="SIMPLE_PINHOLE", flags=0, tz=-4.0),
    Case("behind_radial_pose_frame4", flags=0, frame=4, tz=-4.5),
    # --- terminations
    Case("cap_3", opt=_o(max_num_iterations=3), twin="easy_radial_fk"),
    Case("cap_0", opt=_o(max_num_iterations=0), twin="easy_radial_fk"),
    Case("gradient_at_0", opt=_o(gradient_tolerance=1e6), twin="easy_radial_fk"),
    Case("parameter_exit_pose", flags=0, opt=_o(function_tolerance=0.0, gradient_tolerance=1e-12), twin="easy_radial_pose"),
    Case("parameter_tolerance_coarse", opt=_o(parameter_tolerance=1e-4), twin="easy_radial_fk"),
    Case("function_tolerance_coarse", opt=_o(function_tolerance=1e-2), twin="easy_radial_fk"),
    Case("radius_at_0", opt=_o(initial_trust_region_radius=1e-3, min_trust_region_radius=1e-2), twin="easy_radial_fk"),
    Case("radius_after_shrinking", opt=_o(min_trust_region_radius=1e3), twin="hard_radial_fk", **HARD5),
    # --- inlier counts around the wavefront (64) and the block (256), and below the number of unknowns
    *[Case(f"n{n}_pose", flags=0, n=n) for n in (0, 1, 2, 4, 5, 7, 63, 64, 65, 255, 256, 257)],
    *[Case(f"n{n}_fk", n=n) for n in (0, 1, 2, 3, 5, 7, 63, 64, 65, 255, 256, 257)],
    *[Case(f"n{n}_pinhole_f", model="SIMPLE_PINHOLE", flags=1, n=n) for n in (5, 64, 257)],
    Case("n3_k", flags=2, n=3),
    Case("n4_f", flags=1, n=4),
    *[Case(f"P{P}_pose", flags=0, P=P) for P in (0, 1, 70)],
    *[Case(f"P{P}_fk", P=P) for P in (0, 1, 3, 70)],
    # --- losses
    Case("loss_trivial", loss=0),
    Case("loss_huber", loss=2),
    Case("loss_softl1", loss=3, scale=0.25),
    Case("loss_cauchy_half", scale=0.5),
    Case("loss_cauchy_2_pinhole", model="SIMPLE_PINHOLE", flags=1, scale=2.0),
    # (what the product's callers can set, through AbsolutePoseRefinementOptions: see the wrapper test of the GPU suite)
    Case("loss_cauchy_2", scale=2.0),
    Case("refopts_cap_3_cauchy_2", scale=2.0, opt=_o(gradient_tolerance=1e-3, max_num_iterations=3), twin="loss_cauchy_2"),
    Case("refopts_gradient_cauchy_2", scale=2.0, opt=_o(gradient_tolerance=1e6, max_num_iterations=3), twin="loss_cauchy_2"),
    Case("loss_huber_hard", loss=2, **HARD5),
    Case("loss_softl1_hard", loss=3, scale=0.25, **HARD5),
    Case("loss_trivial_hard", loss=0, **HARD5),
    # --- options, each against its default twin
    Case("max_radius_1e3", opt=_o(max_trust_region_radius=1e3), twin="easy_radial_fk"),
    Case("max_radius_10", opt=_o(max_trust_region_radius=10.0), twin="easy_radial_fk"),
    Case("max_radius_10_hard", opt=_o(max_trust_region_radius=10.0), twin="hard_radial_fk", **HARD5),
    Case("min_lm_diagonal_1", opt=_o(min_lm_diagonal=1.0), twin="easy_radial_fk"),
    Case("min_lm_diagonal_1_hard", opt=_o(min_lm_diagonal=1.0), twin="hard_radial_fk", **HARD5),
    Case("max_lm_diagonal_1e-3", opt=_o(max_lm_diagonal=1e-3), twin="easy_radial_fk"),
    Case("max_lm_diagonal_1e-3_hard", opt=_o(max_lm_diagonal=1e-3), twin="hard_radial_fk", **HARD5),
    Case("initial_radius_10", opt=_o(initial_trust_region_radius=10.0), twin="easy_radial_fk"),
    Case("initial_radius_10_hard", opt=_o(initial_trust_region_radius=10.0), twin="hard_radial_fk", **HARD5),
    # (with the damping taken from diag(J^T J) the Jacobi scaling cancels exactly unless an LM-diagonal clamp bites: the
    #  unscaled solve is paired with a clamp and compared with its scaled twin)
    Case("no_jacobi_min_lm_diagonal_1", opt=_o(jacobi_scaling=0, min_lm_diagonal=1.0), twin="min_lm_diagonal_1"),
    Case("no_jacobi_min_lm_diagonal_1_hard", opt=_o(jacobi_scaling=0, min_lm_diagonal=1.0), twin="min_lm_diagonal_1_hard", **HARD5),
    Case("no_jacobi_max_lm_diagonal_1e-3", opt=_o(jacobi_scaling=0, max_lm_diagonal=1e-3), twin="max_lm_diagonal_1e-3"),
    # (step qualities between 1e-3 and the raised bar exist on these three problems: 0.054, 0.41 and 0.45 .. 0.49)
    Case("min_relative_decrease_0.1_hard", opt=_o(min_relative_decrease=0.1), twin="hard_radial_fk", **HARD5),
    Case("min_relative_decrease_0.5_trivial_hard", loss=0, opt=_o(min_relative_decrease=0.5), twin="loss_trivial_hard", **HARD5),
    Case("min_relative_decrease_0.5_behind", flags=0, frame=4, tz=-4.5, opt=_o(min_relative_decrease=0.5),
         twin="behind_radial_pose_frame4"),
    # --- track precision
    Case("f64_tracks", tracks="f64"),
    Case("f64_tracks_hard_pinhole", model="SIMPLE_PINHOLE", flags=1, tracks="f64", **HARD5),
    # --- non-finite data
    Case("inf_observation", tracks="f64", inf_obs=True),
    Case("inf_observation_f32", model="SIMPLE_PINHOLE", flags=1, inf_obs=True),
    Case("inf_observation_streak_4", tracks="f64", inf_obs=True, opt=_o(max_num_consecutive_invalid_steps=4), twin="inf_observation"),
    Case("nan_point", nan_pt=True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------------------- problems
@functools.lru_cache(maxsize=None)
def _scene(model, P):
    full = P == 800
    return make_scene(S, P, model, shared_camera=False, seed=12, full_visibility=True, outlier_frac=0.05 if full else 0.0)


def default_options():
    """RefineAbsolutePose: Ceres defaults + COLMAP's gradient_tolerance 1.0 (oracle.ba.pose_refinement)."""
    return OB.ceres_options(100, 1e-6, 1.0, 1e-8)


def options_of(case):
    o = default_options()
    for k, v in case.opt:
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def build(case):
    """-> dict: ext0 (S,3,4), q0 (S,4) = the quaternions both solvers start from, t0 (S,3), intr0 (S,4), tracks (S,P,2)
    float32 | float64, points (P,3), mask (S,P) bool, flags (S,) uint8, frame, model, options, loss, scale."""
    sc = _scene(case.model, case.P)
    ext0, K0, extra0, _ = perturb_for_ba(sc, seed=12, **PERTURB[case.pert])
    ext0 = ext0.copy()
    ext0[:, 2, 3] += case.tz
    intr0 = np.zeros((S, 4))
    intr0[:, 0], intr0[:, 1], intr0[:, 2] = K0[:, 0, 0], 512.0, 512.0
    intr0[:, 3] = PINHOLE_INTR3 if extra0 is None else extra0[:, 0]
    f = case.frame
    mask = sc.mask.copy()
    if case.P == 800:
        mask[:, ::7] = False
    if case.n >= 0:
        keep = np.nonzero(mask[f] & ~sc.outlier[f])[0][:case.n]
        assert len(keep) == case.n
        mask[f] = False
        mask[f, keep] = True
    tracks = sc.tracks.copy()
    if case.tracks == "f64":                     # moved by up to 0.45 float32 ulp: the kernel has to read all 64 bits
        dither = np.random.Generator(np.random.PCG64(64)).uniform(-0.45, 0.45, size=tracks.shape)
        tracks = tracks.astype(np.float64) + dither * np.spacing(np.abs(tracks)).astype(np.float64)
        assert not np.array_equal(tracks, tracks.astype(np.float32).astype(np.float64))
    points = sc.points3D.copy()
    first = np.nonzero(mask[f])[0]
    if case.inf_obs:
        tracks[f, first[3], 1] = np.inf
    if case.nan_pt:
        points[first[3], 0] = np.nan
    flags = np.full(S, case.flags, np.uint8)
    return dict(ext0=ext0, q0=np.ascontiguousarray(OB.rotmat_to_quat(ext0[:, :, :3])), t0=np.ascontiguousarray(ext0[:, :, 3]),
                intr0=intr0, tracks=np.ascontiguousarray(tracks), points=points, mask=mask, flags=flags, frame=f,
                model=case.model, options=options_of(case), loss=case.loss, scale=case.scale)


def solve(case, pb=None, points=None, options=None):
    """The oracle's solve of the case's frame -> (ext (3,4), intr (4,), summary with the iteration log).  `points`: other
    3D points (the jitter of `admission`); `options`: another Options struct (the default twin of an option case)."""
    pb = pb or build(case)
    f = pb["frame"]
    return OB.pose_refinement(pb["ext0"][f], pb["tracks"][f], pb["points"] if points is None else points, pb["mask"][f],
                              pb["intr0"][f], pb["model"], refine_focal_length=bool(case.flags & 1),
                              refine_extra_params=bool(case.flags & 2), options=options or pb["options"], loss=pb["loss"],
                              loss_scale=pb["scale"])


@functools.lru_cache(maxsize=None)
def solved(name):
    """(problem, ext, intr, summary) of a table case, solved once per process."""
    pb = build(BY_NAME[name])
    ext, intr, summ = solve(BY_NAME[name], pb)
    return pb, ext, intr, summ


def is_exact_fit(summ):
    """The oracle ends below 1e-9 of its initial cost: a relative bar on the final cost means nothing."""
    return summ["final_cost"] < 1e-9 * summ["initial_cost"]


# ------------------------------------------------------------------------------------------------------------ admission
MARGIN = 1e-6          # the agreement tests/test_oracle_ba_second.py::_compare demands between the two derivations
JITTER, JITTER_SEEDS = 1e-13, (101, 102, 103, 104, 105)


def _clear(value, threshold):
    return abs(value - threshold) > MARGIN * abs(threshold)


def decisions_clear(pb, summ):
    """Admission 1: every decision in the oracle's log is clear of its threshold by MARGIN (relative).  -> list of
    complaints.  The parameter-tolerance threshold needs |x| at every iteration, which the log does not carry: |x| lies
    within the summed step norms of the start's, and the step norm has to clear the whole interval."""
    o, log, bad = pb["options"], summ["iterations"], []
    f = pb["frame"]
    xs = float((pb["q0"][f] ** 2).sum() + (pb["t0"][f] ** 2).sum())
    if summ["n_reduced"] > 6:
        xs += float((pb["intr0"][f, :4 if pb["model"] == "SIMPLE_RADIAL" else 3] ** 2).sum())
    x0, travelled, cost = np.sqrt(xs), 0.0, log[0]["cost"]
    last = len(log) - 1 if summ["termination"] in (2, 3) else -1      # (the iteration a tolerance exit was taken on)
    for i, it in enumerate(log):
        k = it["iteration"]
        if k == 0 or it["successful"]:
            if not _clear(it["gradient_max_norm"], o.gradient_tolerance):
                bad.append(f"iteration {k}: gradient {it['gradient_max_norm']!r} at the tolerance")
        if k > 0 and it["step_norm"] > 0:                       # (an invalid step has no candidate)
            lo = o.parameter_tolerance * (max(x0 - travelled, 0.0) + o.parameter_tolerance) * (1 - MARGIN)
            hi = o.parameter_tolerance * (x0 + travelled + o.parameter_tolerance) * (1 + MARGIN)
            if lo <= it["step_norm"] <= hi and o.parameter_tolerance > 0:
                bad.append(f"iteration {k}: step norm {it['step_norm']!r} inside the parameter-tolerance band [{lo}, {hi}]")
            if not (i == last and summ["termination"] == 3):
                if not _clear(abs(it["cost_change"]), o.function_tolerance * cost):
                    bad.append(f"iteration {k}: cost change {it['cost_change']!r} at the function tolerance")
                if i != last and not _clear(it["relative_decrease"], o.min_relative_decrease):
                    bad.append(f"iteration {k}: step quality {it['relative_decrease']!r} at min_relative_decrease")
            if it["successful"]:
                travelled += it["step_norm"]
        cost = it["cost"]
    return bad


def jitter_stable(case, pb, ext, intr, summ):
    """Admission 2: five solves with the points multiplied by 1 + 1e-13 N(0,1) -> list of complaints."""
    bad = []
    for seed in JITTER_SEEDS:
        rng = np.random.Generator(np.random.PCG64(seed))
        pts = pb["points"] * (1.0 + JITTER * rng.normal(size=pb["points"].shape))
        e, p, s = solve(case, pb, points=pts)
        if any(s[k] != summ[k] for k in INT_KEYS):
            bad.append(f"seed {seed}: summary {[s[k] for k in INT_KEYS]} != {[summ[k] for k in INT_KEYS]}")
            continue
        if not case.finite:
            if e.tobytes() != ext.tobytes() or p.tobytes() != intr.tobytes():
                bad.append(f"seed {seed}: state not bit-identical")
            continue
        de = np.abs(e - ext).max()
        if not de <= 1e-9:
            bad.append(f"seed {seed}: pose moved {de:.2e}")
        if not np.allclose(p, intr, rtol=1e-9, atol=1e-10):
            bad.append(f"seed {seed}: intrinsics moved {np.abs(p - intr).max():.2e}")
        if is_exact_fit(summ):
            if not s["final_cost"] < 1e-9 * s["initial_cost"]:
                bad.append(f"seed {seed}: exact fit lost, final cost {s['final_cost']:.3e}")
        elif not abs(s["final_cost"] - summ["final_cost"]) <= 1e-9 * summ["final_cost"]:
            bad.append(f"seed {seed}: final cost moved {abs(s['final_cost'] / summ['final_cost'] - 1):.2e}")
    return bad


def cost_resolvable(pb, summ):
    """A near fit that is not an exact fit (`is_exact_fit`) is held to the relative 1e-9 on its final cost, so that bar has
    to be wider than the rounding of the data: a residual is a difference of pixel coordinates below 1024, known to one ulp
    of those (2^-43), and one ulp on a residual of r moves r^2 by 2 ulp / r of itself.  The case is out when that exceeds
    half the bar at the RMS residual of the oracle's final cost (every loss here is ~ s for small s)."""
    n = int(pb["mask"][pb["frame"]].sum())
    if n == 0 or is_exact_fit(summ):
        return []
    rms = np.sqrt(2.0 * summ["final_cost"] / (2 * n))
    moved = 2.0 * 2.0 ** -43 / rms
    return [f"one ulp of a pixel moves the final cost by {moved:.1e} of itself (RMS residual {rms:.1e})"] if moved > 0.5e-9 else []


def admission(name):
    """-> list of complaints; empty = the reference alone is stable on the case."""
    case = BY_NAME[name]
    pb, ext, intr, summ = solved(name)
    bad = decisions_clear(pb, summ) + cost_resolvable(pb, summ) if case.finite else []
    return bad + jitter_stable(case, pb, ext, intr, summ)


def differs_from_twin(name):
    """Option cases: True when the oracle's integer summary or final state differs from the twin's (the same problem under
    the twin's options)."""
    case = BY_NAME[name]
    pb, ext, intr, summ = solved(name)
    e2, p2, s2 = solve(case, pb, options=options_of(BY_NAME[case.twin]))
    return (any(summ[k] != s2[k] for k in INT_KEYS) or ext.tobytes() != e2.tobytes() or intr.tobytes() != p2.tobytes())


# ------------------------------------------------------------------------------------------------------- the device entry
def device_options(o):
    from vggsfm_amd import _lib
    return _lib.BAOptions(o.max_num_iterations, o.max_num_consecutive_invalid_steps, o.jacobi_scaling, o.function_tolerance,
                          o.gradient_tolerance, o.parameter_tolerance, o.initial_trust_region_radius,
                          o.max_trust_region_radius, o.min_trust_region_radius, o.min_lm_diagonal, o.max_lm_diagonal,
                          o.min_relative_decrease, 0)


def to_device(a):
    """numpy -> device tensor that always owns memory: an empty array (P = 0) gets a one-element allocation, because the
    entry rejects NULL pointers and an empty torch tensor has one."""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if a.size == 0:
        return torch.zeros(1, dtype=torch.from_numpy(a).dtype, device="cuda")
    return torch.from_numpy(a).cuda()


def run_kernel(cam_q, cam_t, intr, tracks, points, mask, num_rows, P, frame_ids, flags, model, options, loss, scale,
               check=True):
    """Raw ``vgg_pose_refine``: cam_q / cam_t / intr are device tensors and are updated in place, exactly as the kernel
    leaves them; tracks (float32 | float64), points, mask, flags are device tensors (None = a NULL pointer), frame_ids a
    list.  -> (return code,
    [summary dict per listed frame, in launch order])."""
    import torch
    from vggsfm_amd import _lib
    L = _lib.lib()
    F = len(frame_ids)
    fid = torch.tensor(list(frame_ids) or [0], dtype=torch.int32, device="cuda")
    size = ctypes.sizeof(_lib.BASummary)
    summ = torch.zeros(max(F, 1) * size, dtype=torch.uint8, device="cuda")
    co = device_options(options)
    is64 = int(tracks is not None and tracks.dtype == torch.float64)
    rc = L.vgg_pose_refine(points, tracks, is64, mask, int(num_rows), int(P), fid, F, cam_q, cam_t, intr, OB.MODEL[model],
                           flags, ctypes.byref(co), int(loss), scale, summ, _lib.stream_ptr())
    if check:
        _lib.check(rc, "vgg_pose_refine")
    raw = summ.cpu().numpy().tobytes()
    sums = []
    for i in range(F):
        s = _lib.BASummary.from_buffer_copy(raw[i * size:(i + 1) * size])
        sums.append(dict(frame=int(frame_ids[i]), initial_cost=s.initial_cost, final_cost=s.final_cost,
                         **{k: getattr(s, k) for k in INT_KEYS}))
    return rc, sums


def run_rows(q0, t0, intr0, tracks, points, mask, flags, frame_ids, model, options, loss, scale):
    """`run_kernel` on host arrays -> (cam_q, cam_t, intr as the kernel left them, summaries)."""
    q, t, i = to_device(q0), to_device(t0), to_device(intr0)
    _, sums = run_kernel(q, t, i, to_device(tracks), to_device(points), to_device(mask), mask.shape[0], mask.shape[1],
                         frame_ids, to_device(flags), model, options, loss, scale)
    return q.cpu().numpy(), t.cpu().numpy(), i.cpu().numpy(), sums


def run_case(name):
    """The case's own launch: its whole scene on the device, its frame alone in `frame_ids`."""
    pb = solved(name)[0]
    return run_rows(pb["q0"], pb["t0"], pb["intr0"], pb["tracks"], pb["points"], pb["mask"], pb["flags"], [pb["frame"]],
                    pb["model"], pb["options"], pb["loss"], pb["scale"])
