"""The multi-view entries (vggx_multiview_triangulate, vggx_max_tri_angle, vggx_tri_angle_table, vggx_tri_angle_pairs,
vggx_view_centers, vggx_angular_error) on poisoned, guard-banded memory, in the form of
tests/test_gpu_poisoned_track_video.py: the parity cases of tests/test_gpu_multiview.py run with every ``empty``-family
buffer (points, flags, angle tables and the centre workspace among them) filled with 0x00, 0xFF and 0x7F and framed by
guard bands; what they read back must be run-to-run deterministic, bit-identical across the patterns, and no guard byte
may change."""
import pytest

from tests import test_gpu_multiview as TMV
from tests.test_gpu_poisoned_memory import _check_poisoned

pytestmark = pytest.mark.gpu

CASES = {
    # lean form (shared cameras, reduced angles), namesake (per-point cameras, the table), the reduced pass alone
    "bool_mask": lambda mp: TMV.test_lean_and_namesake_equal_the_reference("bool_s8"),
    "float_weights": lambda mp: TMV.test_lean_and_namesake_equal_the_reference("float_s8"),
    "two_views": lambda mp: TMV.test_lean_and_namesake_equal_the_reference("two_views"),
    "f32": lambda mp: TMV.test_float32_and_float64_observations_of_the_same_values_give_the_same_bits(),
    # launches whose last wavefront is partly empty
    "splits": lambda mp: TMV.test_any_split_into_launches_and_any_repetition_gives_the_same_bits("bool_s8"),
    "from_tracks": lambda mp: TMV.test_from_tracks_equals_the_reference(),
    # per-candidate mode with the early-exit flag pass
    "local_refinement_1": lambda mp: TMV.test_local_refinement_equals_the_reference("lr_lo1"),
    "local_refinement_50": lambda mp: TMV.test_local_refinement_equals_the_reference("lr_lo50"),
    # NaN points: written, not left over
    "degenerate": lambda mp: TMV.test_points_with_fewer_than_two_weighted_views_are_nan_and_invalid(),
    "angle_tables": lambda mp: TMV.test_angle_functions_equal_the_reference(),
    "angular_error": lambda mp: TMV.test_angular_error_equals_the_reference(),
}


@pytest.mark.parametrize("name", list(CASES))
def test_multiview_entries_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
