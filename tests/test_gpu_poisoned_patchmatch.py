"""The PatchMatch entries on poisoned, guard-banded memory: cases of tests/test_gpu_patchmatch.py through the checks of
tests/test_gpu_poisoned_memory.py (bit-identical read-backs across 0x00 / 0xFF / 0x7F, no guard byte changed, the cases'
own assertions under every pattern).  21 x 35 is no multiple of the 32 x 16 tile and has an odd width, so its guarded
stores and the checkerboard's right edge are what matter; every entry runs: plane_init (with and without normals, with
holes), plane_cost, step, outputs, and the whole call."""
import pytest

from tests import test_gpu_patchmatch as TP
from tests.test_gpu_poisoned_memory import _check_poisoned

pytestmark = pytest.mark.gpu

CASES = {
    "every_entry_21x35": lambda mp: TP.test_every_half_iteration_matches_restatement("k08_21x35"),
    "plane_cost_21x35": lambda mp: TP.test_plane_cost_of_fronto_parallel_planes_is_the_sweeps_cost_volume("k08_21x35"),
    "holes_and_normals": lambda mp: (TP.test_every_half_iteration_matches_restatement("holes"),
                                     TP.test_every_half_iteration_matches_restatement("normals")),
    "invalid_everywhere": lambda mp: (TP.test_every_half_iteration_matches_restatement("facing_away"),
                                      TP.test_every_half_iteration_matches_restatement("constant_reference")),
    "r1_r3_M8": lambda mp: (TP.test_every_half_iteration_matches_restatement("r1"),
                            TP.test_every_half_iteration_matches_restatement("r3"),
                            TP.test_every_half_iteration_matches_restatement("M8")),
}


@pytest.mark.parametrize("name", list(CASES))
def test_patchmatch_entry_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
