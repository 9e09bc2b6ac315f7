"""The nearest-neighbour entries on poisoned, guard-banded memory: cases of tests/test_gpu_nearest.py through the checks of
tests/test_gpu_poisoned_memory.py (bit-identical read-backs across 0x00 / 0xFF / 0x7F, no guard byte changed, the cases' own
assertions under every pattern).  Every output is allocated by torch.empty, so only what the entries wrote may come back:
M = 255 and 257 are no multiple of the 256 lanes of a workgroup (the guarded stores matter), the no-ops (N = 0, F = 0) must
still write 'none' to every query, the outputs that are off (count inside the library, closest) must leave nothing behind,
and the skippable faces load nothing at their bad rows."""
import pytest

from tests import test_gpu_nearest as TN
from tests.test_gpu_poisoned_memory import _check_poisoned

pytestmark = pytest.mark.gpu

CASES = {
    "m255_m257": lambda mp: (TN.test_nearest_point_matches_restatement("m255"), TN.test_nearest_point_matches_restatement("m257"),
                             TN.test_nearest_face_matches_restatement("plane_255"),
                             TN.test_nearest_face_matches_restatement("plane_257")),
    "no_ops": lambda mp: (TN.test_nearest_point_matches_restatement("n0"), TN.test_nearest_point_matches_restatement("m0"),
                          TN.test_nearest_face_matches_restatement("f0")),
    "outputs_off": lambda mp: (TN.test_nearest_face_matches_restatement("f1"), TN.test_radius_outlier_removal_matches_restatement(),
                               TN.test_distance_stats_are_exact_in_counts_bounded_in_sums_and_reproducible()),
    "skippable_faces": lambda mp: (TN.test_nearest_face_matches_restatement("skippable"),
                                   TN.test_nearest_point_matches_restatement("nonfinite")),
}


@pytest.mark.parametrize("name", list(CASES))
def test_nearest_entry_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
