"""The EPnP entries (vggp_epnp_solve, vggp_pose_score, vggp_epnp_lo, and vgg_p3p_ransac as the LO tests call it) on
poisoned, guard-banded memory, in the form of tests/test_gpu_poisoned_essential.py: the cases of tests/test_gpu_pnp.py run
with every ``empty``-family buffer (R, T, errors, x_cam, winners, flags, counts, residual sums and masks among them) filled
with 0x00, 0xFF and 0x7F and framed by guard bands; what they read back must be run-to-run deterministic, bit-identical
across the patterns, and no guard byte may change."""
import pytest

from tests import test_gpu_pnp as TP
from tests.test_gpu_poisoned_memory import _check_poisoned

pytestmark = pytest.mark.gpu


def _fresh(test, *args):
    """(the LO scene's device results are cached by the tests: every poisoned run makes its own)"""
    def case(mp):
        TP._lo.cache_clear()
        try:
            test(*args)
        finally:
            TP._lo.cache_clear()
    return case


CASES = {
    # a workgroup's worth of points and less, a wavefront and a workgroup crossed, masks, one candidate only
    "solver_clean_5": _fresh(TP.test_solver_equals_the_cpu_candidate, "clean_5"),
    "solver_noisy_257": _fresh(TP.test_solver_equals_the_cpu_candidate, "noisy_257"),
    "solver_masked": _fresh(TP.test_solver_equals_the_cpu_candidate, "masked_6_of_40"),
    "solver_skip_quadratic": _fresh(TP.test_solver_equals_the_cpu_candidate, "skip_quadratic"),
    "independence": _fresh(TP.test_a_problem_is_a_function_of_itself, "masked_half"),
    "shared_points": _fresh(TP.test_shared_points_equal_per_problem_points),
    "masked_out_slots": _fresh(TP.test_nothing_of_a_masked_out_slot_reaches_the_result),
    # every output slot of a problem that is not solved is written, not left over
    "unsolvable": _fresh(TP.test_three_weighted_points_are_flagged_and_every_slot_is_written),
    "planar": _fresh(TP.test_planar_scene_is_finite_or_flagged),
    "efficient_pnp": _fresh(TP.test_efficient_pnp_returns_the_reference_tuple_in_the_input_dtype),
    "local_optimisation": _fresh(TP.test_local_optimisation_equals_the_restatement),
    "zero_rounds": _fresh(TP.test_zero_rounds_return_the_pose_bit_for_bit_with_its_recomputed_support),
    "nothing_found": _fresh(TP.test_nothing_found_and_five_inliers),
    "pose_score": _fresh(TP.test_pose_score_equals_the_numpy_scoring),
    "whole_flow": _fresh(TP.test_whole_flow_with_and_without_local_optimisation),
}


@pytest.mark.parametrize("name", list(CASES))
def test_pnp_entries_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
