"""The intermediates of one Levenberg-Marquardt iteration of the HIP bundle adjustment against a long-double reference
(tests/ba_system_cases.py, itself pinned to the C oracle by tests/test_ba_system_cases.py): reduce buffer 0 (per-camera U, g,
cost) after vgg_ba_begin, reduce buffers 1 (S | rhs) and 2 (the points' gradient maximum) after phase 1 and BEFORE phase 2 --
which factorises S in place and only then puts the unit diagonal on the inactive columns --, and the committed state and log
entry 1 after phases 2 and 3.  The trajectory tests cannot see an error in S: the candidate's cost is second-order
insensitive to the step and the converged state depends on the gradient only.

Measures: S element error / sqrt(S_ii S_jj) with the REFERENCE's diagonal, lower triangle, active rows and columns; U alike
per camera; g, rhs relative to the largest reference element; the step per block type (rotation through log(q_new q_old^-1))
relative to the largest component of the reference's step of that type.  Bound of a quantity on a case = 100 x the deviation
of the float64 CPU evaluation of the reference's formulas from their long-double evaluation on that case, at least 1e-13 for
the sums (buffers 0..2) and 1e-11 for the step; costs 1e-13.  Sign: S y = rhs with rhs = + J_c^T r - ..., the step is -y o scale.

What phase 1 leaves on an inactive row / column j (constant pose or translation component, a frame without observations, a
constant intrinsics block): its Jacobian column is zero, so S[j][j] = min_lm_diagonal / radius exactly (the damping of a zero
column), every other element of row and column j is zero, rhs[j] = 0.  The strict upper triangle stays zero.

Measured on an MI355X over the 15 cases and the 15 variant runs (30 runs, 9 s together): the run that comes closest to its
bound, as GPU deviation / bound, and the largest deviation where that is another run.  The GPU is nowhere further from the
long-double reference than four times the float64 CPU evaluation, and mostly nearer.
  U                  2.4e-14 / 1.0e-13  (h, Cauchy: the kernel's corrector against sqrt(rho'))
  g                  4.6e-15 / 1.0e-13  (c)
  cost               4.3e-15 / 1.0e-13  (e)
  S                  2.2e-14 / 1.2e-12  (a);   largest 1.7e-13 / 3.0e-11  (h)
  rhs                4.1e-15 / 1.7e-13  (k);   largest 1.7e-14 / 2.2e-12  (l_env)
  gmax_pts           2.2e-15 / 1.0e-13  (l_env)
  rotation           2.1e-12 / 1.1e-10  (a)
  translation        3.0e-13 / 1.0e-11  (a);   largest 7.8e-13 / 8.0e-11  (d)
  intrinsics         3.4e-13 / 2.3e-11  (a);   largest 4.8e-11 / 2.9e-07  (l: a focal step of 1e-4 of a focal length of 1e3)
  points             1.4e-12 / 7.7e-11  (a)
  cost_x             1.1e-15 / 1.0e-13  (c)
  cost_cand          1.5e-12 / 2.9e-10  (l)
  cost_change        1.1e-12 / 2.1e-10  (l)
  step_norm          3.2e-13 / 2.0e-11  (a);   largest 1.3e-12 / 2.2e-09  (l_env)
  relative_decrease  1.1e-12 / 2.1e-10  (l)
With a wrong work list on case d (measured once, not a test): one presence bit of a quad cleared -- a 16-row block skipped
that has a camera -- S is off by 3.6e-3, one entry of a tile left out by 1.0e-2; rhs, which does not come from that tile, stays."""
import numpy as np
import pytest
import torch

from tests import ba_system_cases as SC
from tests.test_gpu_ba_glue import CTL_MERGED_GLUE, ctl_int
from vggsfm_amd import _lib
from vggsfm_amd import ba as BA
from vggsfm_amd.dist import ShardedBA

pytestmark = pytest.mark.gpu

LEGACY_GLUE = 4
VARIANTS = ("cam_rhs", "legacy_glue", "separate_tiles", "lanes8", "lanes64")
RUNS = [(name, "default") for name in SC.CASES] + [(name, v) for name in SC.VARIANT_CASES for v in VARIANTS]


def _one_iteration(prob, opt):
    """begin, phases 0..3 and finish on one rank without collectives; the buffers read where they are complete."""
    s = ShardedBA(prob, opt)
    s.begin()
    b0 = s.bufs[0].cpu().numpy().copy()
    s._phase(0)
    s._phase(1)
    b1, b2 = s.bufs[1].cpu().numpy().copy(), s.bufs[2].cpu().numpy().copy()
    s._phase(2)
    s._phase(3)
    summ = s.finish(opt.solver_options.max_num_iterations + 2)
    state = tuple(t.cpu().numpy().copy() for t in (prob.cam_q, prob.cam_t, prob.intr, prob.pts))
    return b0, b1, b2, summ, state, ctl_int(s.ws, CTL_MERGED_GLUE)


@pytest.mark.parametrize("name,variant", RUNS)
def test_intermediates_match_the_reference(name, variant, monkeypatch):
    case = SC.CASES[name]
    opt = SC.options_of(case)
    L = _lib.lib()
    try:
        if variant == "cam_rhs":                    # right-hand side from the camera pass
            assert L.vgg_ba_set_tile_rhs(0) == 0
        elif variant == "legacy_glue":              # tile sums, assembly and preparation as separate launches
            assert L.vgg_ba_set_tile_rhs(2 | LEGACY_GLUE) == 0
        elif variant == "separate_tiles":           # off-diagonal and diagonal tiles in two launches
            monkeypatch.setattr(BA, "MERGED_TILE_MAX_OBS", 0)
        elif variant.startswith("lanes"):
            assert L.vgg_ba_tuning(int(variant[5:]), -1, 0, 0) == 0
        prob = SC.compile_case(name, "cuda")
        SC.check_edges(name, prob, merged=variant != "separate_tiles")
        arrays = SC.host_arrays(prob, case)
        R = SC.reference(name, arrays)
        b0, b1, b2, summ, state, glue = _one_iteration(prob, opt)
    finally:
        L.vgg_ba_set_tile_rhs(2)
        L.vgg_ba_tuning(0, -1, 0, 0)
    ref, pb, so, bounds = R.ref, R.pb, R.so, R.bounds
    C, n, BD = pb.C, pb.n_red, 6 + pb.kd
    # which glue ran: the merged launch needs the tile right-hand side, a diagonal tile in every camera group and no selector
    assert glue == (1 if variant not in ("cam_rhs", "legacy_glue") and name != "g" else 0)
    got, exact = {}, []

    # --- reduce buffer 0
    assert b0.size == C * (BD * BD + BD + 1)
    U, g, cost = b0[:C * BD * BD].reshape(C, BD, BD), b0[C * BD * BD:C * (BD * BD + BD)].reshape(C, BD), b0[C * (BD * BD + BD):]
    got["U"] = max(SC.normalised_error(U[c], ref.U[c], np.diag(ref.U[c]).astype(np.float64)) for c in range(C))
    got["U"] = max(got["U"], max(SC.normalised_error(U[c].T, ref.U[c], np.diag(ref.U[c]).astype(np.float64)) for c in range(C)))
    got["g"] = SC.relative_to_max(g, ref.g)
    got["cost"] = SC.relative_to_max(cost, ref.cost)
    zero = np.array([np.diag(ref.U[c]) == 0 for c in range(C)])               # constant / unobserved columns of a camera's block
    exact.append(("buffer 0: masked columns are zero", bool((U[zero] == 0).all() and (U.transpose(0, 2, 1)[zero] == 0).all()
                                                            and (g[zero] == 0).all())))
    # --- reduce buffer 1
    assert b1.size == n * n + n
    S, rhs = b1[:n * n].reshape(n, n), b1[n * n:]
    act = pb.active[:n]
    ina = np.nonzero(~act)[0]
    got["S"] = SC.normalised_error(S, ref.S, np.where(act, np.diag(ref.S), 0).astype(np.float64))
    got["rhs"] = SC.relative_to_max(rhs[act], ref.rhs[act])
    exact.append(("buffer 1: strict upper triangle is zero", bool((np.triu(S, 1) == 0).all())))
    off = S.copy()
    off[np.arange(n), np.arange(n)] = 0
    exact.append(("buffer 1: inactive rows and columns are zero off the diagonal", bool((off[ina] == 0).all() and (off[:, ina] == 0).all())))
    exact.append(("buffer 1: inactive diagonal = min_lm_diagonal / radius",
                  bool((S[ina, ina] == so.min_lm_diagonal / so.initial_trust_region_radius).all())))
    exact.append(("buffer 1: inactive right-hand side is zero", bool((rhs[ina] == 0).all())))
    exact.append(("inactive columns as the case expects", len(ina) == _expected_inactive(name, case)))
    # --- reduce buffer 2
    got["gmax_pts"] = abs(b2[0] - float(ref.gmax_pts)) / float(ref.gmax_pts)
    # --- the step
    assert len(summ["iterations"]) == 2
    it0, it = summ["iterations"]
    exact.append(("the step is accepted", bool(it["successful"]) and summ["num_successful_steps"] == 1))
    got.update(SC.step_errors(pb, R.x0, state, ref.cand))
    for k in ("cost_change", "step_norm", "relative_decrease"):
        got[k] = abs(it[k] - float(getattr(ref, k))) / abs(float(getattr(ref, k)))
    got["cost_x"] = abs(it0["cost"] - float(ref.cost_x)) / float(ref.cost_x)
    got["cost_cand"] = abs(it["cost"] - float(ref.cost_cand)) / float(ref.cost_cand)
    print(f"\n{name} / {variant}: n = {n}, {len(pb.obs_cam)} observations, {len(ina)} inactive columns, reference in {R.seconds:.1f} s")
    for k, v in got.items():
        print(f"  {k:18s} GPU {v:9.2e}   float64 CPU {R.dev[k]:9.2e}   bound {bounds[k]:9.2e}" + ("   EXCEEDED" if not v <= bounds[k] else ""))
    for what, ok in exact:
        assert ok, what
    over = {k: (v, bounds[k]) for k, v in got.items() if not v <= bounds[k]}
    assert not over, over


def _expected_inactive(name, case):
    """Inactive columns of the reduced system: the gauge (pose 0, t_x of camera 1) or the constant poses; the frames without
    observations of case g."""
    if case.const_poses is not None:
        return 6 * len(case.const_poses)
    return 7 + (6 * 16 if name == "g" else 0)
