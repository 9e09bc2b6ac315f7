"""The essential-matrix entries (vgge_emat_five_point, vgge_emat_solve, vgge_emat_score, vgge_emat_refine, and
vgg_fmat_residuals as estimate_essential calls it) on poisoned, guard-banded memory, in the form of
tests/test_gpu_poisoned_multiview.py: the cases of tests/test_gpu_essential.py run with every ``empty``-family buffer
(candidates, flags, counts, residual sums and residuals among them) filled with 0x00, 0xFF and 0x7F and framed by guard
bands; what they read back must be run-to-run deterministic, bit-identical across the patterns, and no guard byte may
change."""
import pytest

from tests import test_gpu_essential as TE
from tests.test_gpu_poisoned_memory import _check_poisoned

pytestmark = pytest.mark.gpu

CASES = {
    "minimal_solver": lambda mp: TE.test_minimal_solver_equals_the_cpu_solver(),
    # a sample table that is no multiple of the four samples of a wavefront; samples that are flagged, not solved
    "degenerate": lambda mp: TE.test_degenerate_samples_are_finite_or_flagged(),
    "five_matches": lambda mp: TE.test_two_real_roots_and_five_matches_exactly(),
    # all ten slots of a refinement without inliers are written, not left over
    "local_optimisation": lambda mp: TE.test_local_optimisation_needs_five_inliers(),
    "run_5point": lambda mp: TE.test_run_5point_on_many_masked_matches(),
    "flow_equal": lambda mp: TE.test_whole_flow_equals_the_reference_flow("flow_equal"),
    "flow_mixed": lambda mp: TE.test_whole_flow_equals_the_reference_flow("flow_mixed"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_essential_entries_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
