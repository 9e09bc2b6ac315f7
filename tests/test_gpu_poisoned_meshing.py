"""The meshing entries on poisoned, guard-banded memory: cases of tests/test_gpu_meshing.py through the checks of
tests/test_gpu_poisoned_memory.py (bit-identical read-backs across 0x00 / 0xFF / 0x7F, no guard byte changed, the cases' own
assertions under every pattern).  The masks, the offsets, the groups' counts and the mesh are allocated by torch.empty, so
only what the entries wrote may come back: the 9 x 7 x 5 grid (315 nodes) and the 13 x 11 x 10 grid are no multiple of the 256
nodes of a group (their guarded stores matter), the empty mesh returns nothing of the one row it allocates, and a volume
without colour leaves the colour output alone."""
import pytest

from tests import test_gpu_meshing as TM
from tests.test_gpu_poisoned_memory import _check_poisoned

pytestmark = pytest.mark.gpu

CASES = {
    "integrate_21x35_into_9x7x5": lambda mp: (TM.test_integration_and_mesh_match_restatement("k08_21x35_small"),
                                              TM.test_integration_and_mesh_match_restatement("weights_zeros")),
    "empty_mesh": lambda mp: (TM.test_integration_and_mesh_match_restatement("all_zero"),
                              TM.test_extraction_matches_restatement("all_inside"),
                              TM.test_extraction_matches_restatement("all_outside")),
    "outputs_off": lambda mp: (TM.test_integration_and_mesh_match_restatement("no_frames"),
                               TM.test_extraction_matches_restatement("sphere_no_colour"),
                               TM.test_frames_without_colour_volume_and_colour_volume_without_frames()),
    "holes_and_capacity": lambda mp: (TM.test_extraction_matches_restatement("holes"), TM.test_extraction_matches_restatement("tiny"),
                                      TM.test_a_row_beyond_the_capacity_is_not_written()),
}


@pytest.mark.parametrize("name", list(CASES))
def test_meshing_entry_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
